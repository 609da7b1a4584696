"""Model container: the log_prob / sample loops over a list of flows.
Reference: normflow/core.py - NormalizingFlow.log_prob :170-183, .sample
:144-168, save/load :185-197.

Layers that expose ``inverse_into`` / ``forward_into`` add their log|det|
straight into the running ``log_q`` inside the coupling kernel (one [B] buffer
for the whole stack, no per-layer allocation or add); every other Flow goes
through the plain ``(z, log_det)`` contract.

Training objectives (forward_kld / reverse_kld / reverse_alpha_div) differentiate through
vcnf_amd.autograd (the spline VJP kernel).  The fork's
categorical-dequantisation branch (core.py:13-30, :42-54, :157-165) is the
published algorithm per column (vcnf_amd/nets/varquant.py): the fork's file is
not available, so no parity with it is claimed.  ``categoricals`` is always
defined (None without categorical columns) so ``sample`` follows core.py:150-155
instead of failing with the AttributeError the reference has at this HEAD
(SURVEY 8b).
"""
import torch
from torch import nn

from .flows.affine.coupling import AffineCouplingBlock, MaskedAffineFlow, AffineConstFlow
from . import fused_affine, fused, fused_masked, fused_planar, fused_stochastic, vae_ends
from .distributions.encoder import Dirac
from .flows.mixing import Permute
from .flows.neural_spline.wrapper import CoupledRationalQuadraticSpline
from .flows.planar import Planar
from .flows.radial import Radial
from .flows.stochastic import HamiltonianMonteCarlo
from .stacks import refresh_packed
from .transforms import Logit

# The single-launch families, tried in this order at every position of a pass: (the model's switch, the flow types a
# run can start with, the family's planner - the contract is the docstring of vcnf_amd.stacks)
_STACKS = (('fuse_affine_stacks', (Permute, AffineCouplingBlock), fused_affine.stack_run),
           ('fuse_masked_stacks', (MaskedAffineFlow, AffineConstFlow), fused_masked.stack_run),
           ('fuse_rqs_stacks', (CoupledRationalQuadraticSpline,), fused.stack_run),
           ('fuse_planar_stacks', (Planar, Radial), fused_planar.stack_run),
           ('fuse_stochastic_stacks', (HamiltonianMonteCarlo,), fused_stochastic.stack_run))


class _PackedWeightsMixin:
    """Keeps the packed weight copies of the fused kernels honest across the events that change parameters
    behind autograd's back: train() / eval() transitions and load_state_dict() drop the caches
    (vcnf_amd.stacks.refresh_packed); after a manual ``p.data`` edit call ``refresh_packed()`` yourself."""

    def _install_pack_hooks(self):
        self.register_load_state_dict_post_hook(lambda module, incompatible: refresh_packed(module) and None)

    def train(self, mode=True):
        refresh_packed(self)
        return super().train(mode)

    def refresh_packed(self):
        return refresh_packed(self)


class _FlowWalks:
    """The passes over ``self.flows`` that NormalizingFlow and NormalizingFlowVAE share, and the switches of the
    single-launch families they consult."""

    def _init_stack_switches(self):
        self.fuse_affine_stacks = True           # runs of one-kernel affine layers in a single launch (fused_affine.run_stack)
        self.fuse_rqs_stacks = True              # runs of one-kernel RQS layers in a single launch: long runs at small batches, pairs above (fused.run_stack)
        self.fuse_masked_stacks = True           # runs of MaskedAffineFlow (+ MLP conditioners) / ActNorm layers in a single launch
        self.fuse_planar_stacks = True           # runs of Planar / Radial layers in a single launch (fused_planar.run)
        self.fuse_stochastic_stacks = True       # runs of HamiltonianMonteCarlo layers in a single launch (fused_stochastic.run)

    def _stack_at(self, order, i, z, context, density, differentiable=False):
        """(end, launch) of the first family of _STACKS that is switched on and plans a run from order[i], or None;
        ``differentiable``: only the families whose planner is marked so (vcnf_amd.stacks)."""
        for switch, starts, stack_run in _STACKS:
            if isinstance(order[i], starts) and getattr(self, switch) and \
                    (not differentiable or getattr(stack_run, 'differentiable', False)):
                run = stack_run(self, order, i, z, context, density)
                if run is not None:
                    return run
        return None

    def _walk(self, z, log_q, context, density):
        """(z, log_q) after one pass over the flows: last to first through their inverses with the log-dets added
        (``density``), or first to last with the log-dets subtracted (sampling).  At each position the first of these
        takes the layers it covers: a single-launch run of one family (_STACKS, in order), a one-kernel affine layer
        and the Permute after it in model order, the layer's accumulating form (inverse_into / forward_into), the
        plain (z, log_det) contract."""
        order = list(reversed(self.flows)) if density else list(self.flows)
        sign = 1.0 if density else -1.0
        n = len(order)
        i = 0
        while i < n:
            flow = order[i]
            run = self._stack_at(order, i, z, context, density)
            if run is not None:
                i, launch = run
                z, log_q = launch(z, log_q, sign)
                continue
            # the Permute becomes the affine kernel's load index in the density pass, its store index when sampling
            if i + 1 < n:
                block, perm = (order[i + 1], flow) if density else (flow, order[i + 1])
                if isinstance(block, AffineCouplingBlock) and isinstance(perm, Permute) and z.dim() == 2 \
                        and block.fusable(z):
                    gather = perm._idx32(density, z.device)
                    z = block.run_with_permute(z, density, log_q, sign, in_gather=gather if density else None,
                                               out_gather=None if density else gather)
                    i += 2
                    continue
            ctx = {'context': context} if (context is not None and getattr(flow, 'takes_context', False)) else {}
            into = getattr(flow, 'inverse_into' if density else 'forward_into', None)
            if into is not None:
                z = into(z, log_q, **ctx)
            elif density:
                z, log_det = flow.inverse(z, **ctx)
                log_q += log_det
            else:
                z, log_det = flow(z, **ctx)
                log_q -= log_det
            i += 1
        return z, log_q

    def _plain_walk(self, z, log_q, context, density, trace=None):
        """The pass of ``_walk`` through every flow's plain ``(z, log_det)`` contract, log-dets summed out of place;
        ``trace``: two lists that receive each layer's output and log-det as numpy arrays (the reference's
        ``extended`` lists).  Without a trace a family of _STACKS whose ``stack_run.differentiable`` is set - its run is one
        autograd node and returns the log-dets out of place when given no log_q - still takes its runs in one launch:
        reverse_kld trains through here."""
        order = list(reversed(self.flows)) if density else list(self.flows)
        i = 0
        while i < len(order):
            flow = order[i]
            run = self._stack_at(order, i, z, context, density, True) if trace is None else None
            if run is not None:
                i, launch = run
                z, log_det = launch(z, None, 1.0 if density else -1.0)
                log_q = log_q + log_det
                continue
            ctx = {'context': context} if (context is not None and getattr(flow, 'takes_context', False)) else {}
            z, log_det = flow.inverse(z, **ctx) if density else flow(z, **ctx)
            if trace is not None:
                trace[0].append(z.detach().cpu().numpy())
                trace[1].append(torch.as_tensor(log_det).detach().cpu().numpy())
            log_q = log_q + log_det if density else log_q - log_det
            i += 1
        return z, log_q


def _int_list(values, name, lowest, distinct=False):
    """``values`` as a list of ints >= ``lowest`` (``distinct``: no value twice), or a ValueError naming the argument."""
    try:
        listed = list(values)
    except TypeError:
        raise ValueError("%s must be a sequence of ints, got %r" % (name, values)) from None
    if any(isinstance(v, bool) or not isinstance(v, int) or v < lowest for v in listed):
        raise ValueError("%s must hold ints >= %d, got %r" % (name, lowest, listed))
    if distinct and len(set(listed)) != len(listed):
        raise ValueError("%s must hold distinct columns, got %r" % (name, listed))
    return listed


class NormalizingFlow(_PackedWeightsMixin, _FlowWalks, nn.Module):
    """The model container (core.py:13-30).  With ``categoricals`` (column indices of the rows [B, D]) and ``catlevels``
    (their numbers of levels) those columns hold integer codes: ``log_prob`` and ``forward_kld`` dequantise them first and
    add the log-dets, ``sample`` and ``sample_from`` quantise last, both through the ONE dequantiser module ``catvdeqs``
    that covers all categorical columns (None: ``nets.Dequantization()``, uniform noise; ``nets.VariationalDequantization``
    learns the noise - vcnf_amd/nets/varquant.py).  ``reverse_kld`` and ``reverse_alpha_div`` stay on the continuous rows.
    Without categoricals ``categoricals`` is None, there is no ``catvdeqs`` and no pass changes."""

    def __init__(self, q0, flows, p=None, categoricals=None, catlevels=None, catvdeqs=None):
        super().__init__()
        self._install_pack_hooks()
        self.q0 = q0
        self.flows = nn.ModuleList(flows)
        self.p = p
        self.categoricals = None
        self.catlevels = None
        self._init_stack_switches()
        if categoricals is not None or catlevels is not None or catvdeqs is not None:
            self._init_categoricals(categoricals, catlevels, catvdeqs)

    def _init_categoricals(self, categoricals, catlevels, catvdeqs):
        from .nets.varquant import Dequantization
        if categoricals is None:
            raise ValueError("categoricals must be given together with catlevels" if catlevels is not None else
                             "categoricals and catlevels must be given with catvdeqs")
        if catlevels is None:
            raise ValueError("catlevels must be given together with categoricals")
        columns = _int_list(categoricals, "categoricals", 0, distinct=True)
        levels = _int_list(catlevels, "catlevels", 1)
        if len(columns) != len(levels):
            raise ValueError("categoricals and catlevels must have equal lengths, got %d and %d" % (len(columns), len(levels)))
        if isinstance(catvdeqs, (list, tuple)):
            raise TypeError("catvdeqs must be ONE dequantiser module (nets.Dequantization or nets.VariationalDequantization): "
                            "one module covers all categorical columns; the fork's per-column list cannot be restated "
                            "without its source")
        if catvdeqs is None:
            catvdeqs = Dequantization()
        if not (isinstance(catvdeqs, nn.Module) and callable(getattr(catvdeqs, 'dequantize', None))
                and callable(getattr(catvdeqs, 'quantize', None))):
            raise TypeError("catvdeqs must be a module with dequantize and quantize, got %r" % (catvdeqs,))
        self.categoricals, self.catlevels = columns, levels
        self.catvdeqs = catvdeqs

    # ------------------------------------------------------------ categorical columns
    def _need_categoricals(self):
        if self.categoricals is None:
            raise RuntimeError("this model has no categorical columns (categoricals=, catlevels=)")

    def dequantize(self, x, noise=None, log_q=None):
        """(xt, ld): the rows with their categorical columns made continuous, and the log-det that goes with
        ``log q(xt)``.  ``noise``: the uniform draws [B, C]; None draws them.  ``log_q``: add ld into it in place."""
        self._need_categoricals()
        return self.catvdeqs.dequantize(x, self.categoricals, self.catlevels, noise=noise, log_q=log_q)

    def quantize(self, z):
        """(x, ld): continuous rows with their categorical columns turned into integer codes, and the log-det of the
        continuous map in front of the floor (a sampling pass subtracts it)."""
        self._need_categoricals()
        return self.catvdeqs.quantize(z, self.categoricals, self.catlevels)

    def _quantized(self, z, log_q):
        z, log_det = self.catvdeqs.quantize(z, self.categoricals, self.catlevels)
        return z, (log_q - log_det if log_q.requires_grad else log_q.sub_(log_det))

    # ------------------------------------------------------------ density
    def log_prob(self, x, context=None, noise=None):
        """log q(x) [B]: flows inverted last to first, log-dets added, base
        log-density at the end (core.py:176-183).

        With categorical columns this is ONE draw of the variational bound
        ``log P(x) >= E_u[log q(xt) + ld_merge + ld_prepare + ld_varflows]`` and not the log-probability of the codes: a
        stochastic lower bound, different from call to call unless the draws ``noise`` [B, C] are given."""
        log_q = torch.zeros(len(x), dtype=x.dtype, device=x.device)
        if self.categoricals is not None:
            x, log_q = self.catvdeqs.dequantize(x, self.categoricals, self.catlevels, noise=noise, log_q=log_q)
        elif noise is not None:
            self._need_categoricals()
        z, log_q = self._walk(x, log_q, context, True)
        if hasattr(self.q0, 'from_noise'):
            self.q0.log_prob(z, out=log_q)
        else:
            log_q += self.q0.log_prob(z)
        return log_q

    # ------------------------------------------------------------ sampling
    def sample(self, num_samples=1, context=None):
        """(z, log q(z)) for fresh base draws (core.py:150-155, :168).  With categorical columns z holds integer codes
        there and log q is the density of the continuous point in [0, K_c) in front of the floor."""
        z, log_q = self.q0(num_samples)
        z, log_q = self._walk(z, log_q, context, False)
        return (z, log_q) if self.categoricals is None else self._quantized(z, log_q)

    def sample_from(self, eps, context=None):
        """Same as ``sample`` with the standard-normal base draw given."""
        z, log_q = self.q0.from_noise(eps)
        z, log_q = self._walk(z, log_q, context, False)
        return (z, log_q) if self.categoricals is None else self._quantized(z, log_q)

    # ------------------------------------------------------------ objectives
    def _pull(self, z, context=None, trace=None):
        """log q of given points through the plain ``(z, log_det)`` contract, optionally
        recording each layer's output and log-det (the reference's ``extended`` lists)."""
        log_q = torch.zeros(len(z), dtype=z.dtype, device=z.device)
        z, log_q = self._plain_walk(z, log_q, context, True, trace)
        return log_q + self.q0.log_prob(z)

    def forward_kld(self, x, extended=False, context=None, noise=None):
        """-mean log q(x) (core.py:30-65).  ``extended``: also the per-layer latents and
        log-dets as numpy arrays and the per-sample log q; with categorical columns the lists start after the
        dequantisation.  ``noise``: as for ``log_prob``."""
        if not extended:
            return -torch.mean(self.log_prob(x, context, noise))
        trace = ([], [])
        if self.categoricals is not None:
            x, log_det = self.dequantize(x, noise)
            log_q = self._pull(x, context, trace) + log_det
        else:
            log_q = self._pull(x, context, trace)
        return -torch.mean(log_q), trace[0], trace[1], log_q

    def _frozen_log_q(self, z, context):
        """log q(z) with the parameters held constant (core.py:87-95 / :124-131): the path
        derivative estimators differentiate through z only."""
        params = [p for p in self.parameters() if p.requires_grad]
        for p in params:
            p.requires_grad = False
        try:
            return self._pull(z, context)
        finally:
            for p in params:
                p.requires_grad = True

    def reverse_kld(self, num_samples=1, beta=1., score_fn=True, extended=False, context=None):
        """mean log q(z) - beta * mean log p(z), z ~ q (core.py:67-100)."""
        z, log_q = self.q0(num_samples)
        trace = ([], []) if extended else None
        z, log_q = self._plain_walk(z, log_q, context, False, trace)
        if not score_fn:
            log_q = self._frozen_log_q(z, context)
        log_p = self.p.log_prob(z)
        loss = torch.mean(log_q) - beta * torch.mean(log_p)
        if extended:
            return loss, trace[0], trace[1], log_p, log_q
        return loss

    def reverse_alpha_div(self, num_samples=1, alpha=1, dreg=False, extended=False, context=None):
        """Alpha divergence with samples from q (core.py:101-141); ``dreg``: the doubly
        reparametrised estimator."""
        import numpy as np
        z, log_q = self.sample(num_samples, context)
        log_p = self.p.log_prob(z)
        if dreg:
            w_const = torch.exp(log_p - log_q).detach()
            log_q = self._frozen_log_q(z, context)
            # log w = log p - log q as it stands, not log(exp(.)): where exp underflows (fp32 below e^-103; a sharp
            # target such as RingMixture puts samples of an untrained flow there) the weight is 0, log(0) = -inf and
            # the loss their product, NaN
            log_w = log_p - log_q
            w_alpha = w_const ** alpha
            w_alpha = w_alpha / torch.mean(w_alpha)
            weights = (1 - alpha) * w_alpha + alpha * w_alpha ** 2
            loss = -alpha * torch.mean(weights * log_w)
        else:
            loss = np.sign(alpha - 1) * torch.logsumexp(alpha * (log_p - log_q), 0)
        if extended:
            return loss, [], []
        return loss

    # ------------------------------------------------------------ checkpoints
    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, weights_only=True))


class ClassCondFlow(NormalizingFlow):
    """Normalizing flow with a class-conditional base distribution (normflow/core.py:200-268): the loops of
    NormalizingFlow, with the labels ``y`` (int64 [B] or a float matrix [B, num_classes]) given to the base only."""

    def __init__(self, q0, flows):
        super().__init__(q0, flows)

    def log_prob(self, x, y):
        z, log_q = self._walk(x, torch.zeros(len(x), dtype=x.dtype, device=x.device), None, True)
        self.q0.log_prob(z, y, out=log_q)
        return log_q

    def forward_kld(self, x, y):
        """-mean log q(x | y) (core.py:214-231)."""
        return -torch.mean(self.log_prob(x, y))

    def sample(self, num_samples=1, y=None):
        """(z, log q(z | y)); labels are drawn by the base when ``y`` is None (core.py:233-249)."""
        z, log_q = self.q0(num_samples, y)
        return self._walk(z, log_q, None, False)

    def sample_from(self, eps, y=None):
        """``sample`` with the standard-normal base draw given."""
        z, log_q = self.q0.from_noise(eps, y)
        return self._walk(z, log_q, None, False)


class NormalizingFlowVAE(_PackedWeightsMixin, _FlowWalks, nn.Module):
    """VAE with normalizing flows on the latent (normflow/core.py:402-454): an encoder ``q0(x, num_samples)``, flows in
    the sampling direction, a ``prior`` (any object with ``log_prob``: a base distribution of this package or a
    ``torch.distributions`` object) and an optional ``decoder``.  The flows go through NormalizingFlow's plain walk, so a
    stretch of Planar / Radial layers is one launch and one autograd node between the end-cap kernels of
    ``distributions.NNDiagGaussian`` and the decoders (csrc/vae_ends.hip).  Tensors the kernels do not compute on (CPU,
    half precision) take the torch composition of every layer and of the prior that has one."""

    def __init__(self, prior, q0=None, flows=None, decoder=None):
        super().__init__()
        self._install_pack_hooks()
        self.prior = prior
        self.decoder = decoder
        self.flows = nn.ModuleList(flows if flows is not None else [])
        self.q0 = q0 if q0 is not None else Dirac()
        self._init_stack_switches()

    def forward(self, x, num_samples=1):
        """(z [B, S, ...], log q(z | x) [B, S], log p(x, z) [B, S]) for S = num_samples latents per item of x [B, ...]."""
        z, log_q = self.q0(x, num_samples=num_samples)
        z = z.reshape((-1,) + tuple(z.shape[2:]))
        log_q = log_q.reshape(-1)
        if vae_ends.on_kernels(z):
            z, log_q = self._plain_walk(z, log_q, None, False)
            log_p = self.prior.log_prob(z)
        else:
            for flow in self.flows:
                z, log_det = getattr(flow, '_torch_forward', flow)(z)
                log_q = log_q - log_det
            log_p = getattr(self.prior, '_torch_log_prob', self.prior.log_prob)(z)
        if self.decoder is not None:
            log_p = log_p + self.decoder.log_prob(x, z)
        return (z.reshape((-1, num_samples) + tuple(z.shape[1:])), log_q.reshape(-1, num_samples),
                log_p.reshape(-1, num_samples))


class MultiscaleFlow(_PackedWeightsMixin, nn.Module):
    """Multiscale (RealNVP / Glow) container: per level a list of flows, a Merge between
    levels and one base distribution per level.  Reference: normflow/core.py:271-399
    (sample :310-340, log_prob :342-367).  With ``class_cond`` the bases that take labels (GlowBase,
    ClassCondDiagGaussian: ``takes_labels``) are called with ``y``; DiagGaussian bases are called without it."""

    def __init__(self, q0, flows, merges, transform=None, class_cond=True):
        super().__init__()
        self._install_pack_hooks()
        if class_cond and any(not hasattr(q, 'from_noise') for q in q0):
            raise NotImplementedError("a base distribution without from_noise is not supported; use GlowBase, "
                                      "ClassCondDiagGaussian or DiagGaussian bases")
        self.q0 = nn.ModuleList(q0)
        self.num_levels = len(self.q0)
        self.flows = nn.ModuleList([nn.ModuleList(f) for f in flows])
        self.merges = nn.ModuleList(merges)
        self.transform = transform
        self.class_cond = bool(class_cond)

    def forward(self, x, y=None):
        return -self.log_prob(x, y)

    def forward_kld(self, x, y=None):
        """core.py:296-308: forward KL divergence estimate -mean(log_prob); differentiable through the VJP
        kernels of vcnf_amd.autograd."""
        return -torch.mean(self.log_prob(x, y))

    def log_prob(self, x, y=None):
        """core.py:348-367: optional input transform, then per level (finest last) the
        flows inverted, the split-off half scored by that level's base.  ``x`` may be a ``torch.uint8`` batch of image
        bytes when the transform is a ``transforms.Logit``: it is dequantised with fresh uniform noise, scaled and
        transformed in one launch, in the dtype of the first base's ``loc``."""
        log_q = 0
        z = x
        if x.dtype == torch.uint8:
            # image bytes: dequantisation noise, scaling and the transform in one launch (transforms.Logit.inverse_u8)
            if not isinstance(self.transform, Logit):
                raise TypeError("byte input needs transform=vcnf_amd.transforms.Logit(...) to dequantise it; this "
                                "model's transform is %r" % (self.transform,))
            z, log_det = self.transform.inverse_u8(x, dtype=self.q0[0].loc.dtype)
            log_q = log_q + log_det
        elif self.transform is not None:
            z, log_det = self.transform.inverse(z)
            log_q = log_q + log_det
        for i in range(self.num_levels - 1, -1, -1):
            for flow in reversed(self.flows[i]):
                z, log_det = flow.inverse(z)
                log_q = log_q + log_det
            if i > 0:
                [z, z_], log_det = self.merges[i - 1].inverse(z)
                log_q = log_q + log_det
            else:
                z_ = z
            log_q = log_q + (self.q0[i].log_prob(z_, y) if self._labelled(i) else self.q0[i].log_prob(z_))
        return log_q

    def _labelled(self, i):
        """Base ``i`` is called with the labels (core.py:334-337, :361-364)."""
        return self.class_cond and getattr(self.q0[i], 'takes_labels', False)

    def sample(self, num_samples=1, y=None, temperature=None):
        if temperature is not None:
            self.set_temperature(temperature)
        if y is not None:
            num_samples = len(y)
        noise = [torch.randn((num_samples,) + q.shape, dtype=q.loc.dtype, device=q.loc.device) for q in self.q0]
        try:
            return self.sample_from(noise, y)
        finally:
            if temperature is not None:
                self.reset_temperature()

    def sample_from(self, noise, y=None):
        """core.py:320-340 with the per-level standard-normal draws supplied.  A base that takes labels draws its own
        (torch.randint, as in the reference) when ``y`` is None."""
        z, log_q = None, None
        for i in range(self.num_levels):
            z_, log_q_ = self.q0[i].from_noise(noise[i], y) if self._labelled(i) else self.q0[i].from_noise(noise[i])
            if i == 0:
                z, log_q = z_, log_q_
            else:
                log_q = log_q + log_q_
                z, log_det = self.merges[i - 1]([z, z_])
                log_q = log_q - log_det
            for flow in self.flows[i]:
                z, log_det = flow(z)
                log_q = log_q - log_det
        if self.transform is not None:
            z, log_det = self.transform(z)
            log_q = log_q - log_det
        return z, log_q

    def set_temperature(self, temperature):
        for q0 in self.q0:
            if hasattr(q0, 'temperature'):
                q0.temperature = temperature
            else:
                raise NotImplementedError('One base function does not support temperature annealed sampling')

    def reset_temperature(self):
        self.set_temperature(None)

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, weights_only=True))
