"""Host side of csrc/planar_radial.hip: runs of consecutive ``Planar`` / ``Radial`` layers in ONE launch.

``plan`` finds the longest stretch of such layers that share the inputs' feature shape, dtype and device (one layer is
enough for a run; in a density pass only leaky_relu Planar layers have an inverse, so only they form a run and any other
layer is left to raise what its ``inverse`` raises).  ``operands`` turns the run's parameters into the kernel's
effective operands - u_hat, w, b / z_0, |alpha|, beta_eff, one row per layer - with batched torch ops on ``torch.stack``
of the parameters: a fixed number of launches whatever the number of layers, evaluated exactly as the reference writes
the formulas (``log(1 + exp(.))`` included, so overflow behaves as there), and differentiable, so autograd carries the
kernel's operand gradients on to the parameters and nothing of that chain is hand-written.  The operands are rebuilt on
every call: they are [K, D]-sized, and a cache keyed on the parameters' addresses and versions goes stale under graph
replay.  Only what depends on the run's structure alone (the layer kinds, the slopes, the order of the rows) is kept, for
the _STRUCTURE_LIMIT runs used last.  Its first use for a run copies three small tensors to the device, which a graph
capture does not allow: call the model once before capturing it.
"""
import torch

from . import _lib
from .autograd import PlanarRadialStackFn, needs_grad
from .flows.planar import NEGATIVE_SLOPE, Planar
from .flows.radial import Radial
from .stacks import add_log_det

_STRUCTURE = {}               # (kinds, device, dtype) -> see _structure; insertion order is the order of last use
_STRUCTURE_LIMIT = 64


def _kind(flow):
    """The kernel's code for the layer; None for anything else, a subclass included: what it overrides is unknown here,
    so it joins no run and evaluates its own torch composition (``covers`` is False)."""
    if type(flow) is Planar:
        return _lib.PLANAR_TANH if flow.act == "tanh" else _lib.PLANAR_LEAKY
    if type(flow) is Radial:
        return _lib.RADIAL
    return None


def _row(flow):
    return flow.z_0 if isinstance(flow, Radial) else flow.u


def _params(flow):
    return (flow.beta, flow.alpha, flow.z_0) if isinstance(flow, Radial) else (flow.u, flow.w, flow.b)


def covers(flow, z):
    """Whether the kernel evaluates ``flow`` on inputs like ``z``: raises for what the package does not compute at all
    (CPU tensors, other dtypes, parameters elsewhere than the inputs), False beyond the kernel's feature limit."""
    _lib.require_device(z, *_params(flow), f64=True, allow_grad=True)
    row = _row(flow)
    if tuple(z.shape[1:]) != tuple(row.shape[1:]) or z.dim() < 2:
        raise _lib.VcnfError("expected inputs [batch, %s], got %s" % (", ".join(map(str, row.shape[1:])), list(z.shape)))
    if any(p.dtype != z.dtype for p in _params(flow)):
        raise _lib.VcnfError("inputs are %s, the layer's parameters %s" % (z.dtype, row.dtype))
    return _kind(flow) is not None and bool(_lib.lib().vcnf_planar_radial_supported(row.numel()))


def _joins(flow, z, density):
    """``flow`` can be part of a run over inputs like ``z``."""
    kind = _kind(flow)
    if kind is None or (density and kind != _lib.PLANAR_LEAKY):
        return False
    row = _row(flow)
    return tuple(row.shape[1:]) == tuple(z.shape[1:]) and all(p.dtype == z.dtype and p.device == z.device for p in _params(flow))


def plan(order, start, z, density):
    """(end, flows): the longest run order[start:end] one launch evaluates, or None."""
    if z.dim() < 2 or not z.is_cuda or z.dtype not in (torch.float32, torch.float64):
        return None
    if not _lib.lib().vcnf_planar_radial_supported(z[0].numel()):
        return None
    end = start
    while end < len(order) and _joins(order[end], z, density):
        end += 1
    return (end, order[start:end]) if end > start else None


def stack_run(owner, order, start, z, context, density):
    """NormalizingFlow's planner for this family (the contract: vcnf_amd.stacks).  The inverse has no
    differentiable kernel path: a density pass that autograd records takes the layers one by one."""
    p = plan(order, start, z, density)
    if p is None:
        return None
    end, flows = p
    if density and needs_grad(z, *[t for f in flows for t in _params(f)]):
        return None
    return end, lambda z, log_q, sign: run(flows, z, density, log_q, sign)


stack_run.differentiable = True       # NormalizingFlow's plain walk (the one autograd records) takes these runs too


def _structure(kinds, device, dtype):
    """What a run's structure alone decides: the kinds (host and device copies), the slope column of the planar rows and
    the index that puts [planar rows | radial rows] into the order of the layers (None when they are in it already)."""
    key = (kinds, str(device), dtype)
    s = _STRUCTURE.pop(key, None)
    if s is None:
        while len(_STRUCTURE) >= _STRUCTURE_LIMIT:
            del _STRUCTURE[next(iter(_STRUCTURE))]
        planar = [i for i, k in enumerate(kinds) if k != _lib.RADIAL]
        radial = [i for i, k in enumerate(kinds) if k == _lib.RADIAL]
        slope = torch.tensor([NEGATIVE_SLOPE if kinds[i] == _lib.PLANAR_LEAKY else 0.0 for i in planar], dtype=dtype, device=device)
        index = None
        if planar and radial:
            where = {layer: at for at, layer in enumerate(planar + radial)}
            index = torch.tensor([where[i] for i in range(len(kinds))], dtype=torch.int64, device=device)
        s = (_lib.planar_radial_kinds(kinds, device), slope, index)
    _STRUCTURE[key] = s
    return s


def operands(flows, device, dtype):
    """(kinds, va [K, D], vb [K, D], sc [K, 2]) of a run, as include/vcnf_hip.h describes them."""
    kinds = tuple(_kind(f) for f in flows)
    codes, slope, index = _structure(kinds, device, dtype)
    planar = [f for f, k in zip(flows, kinds) if k != _lib.RADIAL]
    radial = [f for f, k in zip(flows, kinds) if k == _lib.RADIAL]
    va, vb, sc = [], [], []
    if planar:
        u = torch.stack([f.u.reshape(-1) for f in planar])
        w = torch.stack([f.w.reshape(-1) for f in planar])
        b = torch.cat([f.b.reshape(1) for f in planar])
        inner = torch.sum(w * u, 1, keepdim=True)
        va.append(u + (torch.log(1 + torch.exp(inner)) - 1 - inner) * w / torch.sum(w ** 2, 1, keepdim=True))
        vb.append(w)
        sc.append(torch.stack([b, slope], 1))
    if radial:
        z_0 = torch.stack([f.z_0.reshape(-1) for f in radial])
        alpha = torch.abs(torch.cat([f.alpha.reshape(1) for f in radial]))
        beta = torch.log(1 + torch.exp(torch.cat([f.beta.reshape(1) for f in radial]))) - alpha
        va.append(z_0)
        vb.append(torch.zeros_like(z_0))
        sc.append(torch.stack([alpha, beta], 1))
    if index is None:
        return codes, va[0], vb[0], sc[0]
    return codes, torch.cat(va).index_select(0, index), torch.cat(vb).index_select(0, index), torch.cat(sc).index_select(0, index)


def run(flows, z, density, log_q, sign):
    """One launch for the run: (z', log_q + sign * log|det|), or (z', sign * log|det|) without a log_q.  With autograd
    recording (sampling direction only) the run is one node, PlanarRadialStackFn, and log_q is not written in place."""
    z2 = z.reshape(len(z), -1)
    codes, va, vb, sc = operands(flows, z.device, z.dtype)
    if needs_grad(z, va, vb, sc):
        if density:
            raise _lib.VcnfError("the leaky_relu inverse has no differentiable kernel path")
        out, ld = PlanarRadialStackFn.apply(z2, va, vb, sc, codes)
        return add_log_det(out.reshape(z.shape), ld, log_q, sign)
    out, log_q = _lib.planar_radial_stack(z2, codes, va, vb, sc, inverse=density, logdet=log_q, sign=sign)
    return out.reshape(z.shape), log_q
