"""The sampling direction of the autoregressive flows in one launch (csrc/made_sample.hip): host side.

``MaskedAffineAutoregressive.inverse`` and ``MaskedPiecewiseRationalQuadraticAutoregressive.inverse`` are, in the
reference, ``features`` full MADE passes that each fix one more variable.  With the MADE's sequential degrees a hidden
unit of degree m depends only on inputs and hidden units of degree <= m, so the passes collapse into one masked pass
ordered by degree with an inversion between stages (the stage rule: include/vcnf_hip.h at vcnf_made_sample_*).  This
module decides whether a layer and a call can take that kernel (``plan``), keeps the operands the kernel reads in place
of the module's parameters (``pack``, a ``vcnf_amd.derived`` slot) and launches it (``run``).

What the kernel reads (``pack``)
    * the masked weights ``W * mask`` of every layer with the hidden units permuted into ascending degree (a stable
      sort, the same permutation in every layer), the input columns and the final layer's row blocks in ascending
      variable degree - one flat buffer, laid out as the header says;
    * int32 tables: the variable order, and per stage the number of hidden units of degree <= the stage;
    * the context layers' weights and biases with their rows in the same unit order (the projections themselves are one
      batched GEMM in ``run``).
    The degrees come from the module's own buffers (the input degrees from ``final_layer.degrees[::multiplier]``, which
    covers ``permute_mask=True``), and every ``mask`` buffer must be elementwise <= the mask its degrees imply (``>=``
    for hidden layers, ``>`` for the output layer): a mask that lets a unit see more is not autoregressive in the order
    the kernel walks, and the layer keeps the loop.  The check runs once per version of the buffers, with the rebuild.

What takes the kernel (``plan``)
    fp32 / fp64 contiguous [B, D] inputs on the device with nothing recording a gradient; ``type(net) is MADE`` with
    residual blocks (none included), ReLU, no batch norm, no preprocessing, dropout inactive; scalar tails; a shape
    ``vcnf_made_sample_supported`` accepts (splines: 8, 10 or 16 bins), outside the two regions where the kernel
    measured level with the loop (``LOOP_FROM_*``).  Everything else - feed-forward blocks, random masks, other activations,
    per-feature tails, half precision, CPU tensors, anything under autograd - takes the loop, unchanged.

The first call of a layer builds the buffers (a few small device kernels and one host read for the mask check): call
the layer once before capturing it into a HIP graph, as for the other single-launch families.
"""
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib, derived
from .nets.made import MADE, MaskedResidualBlock

SLOT = 'made_sample'
# Where the kernel measured level with the loop (profiles/ar_sampling.md) the loop stays: the notebook conditioner or
# larger from 65 536 rows on (0.96 - 1.05 x at (65536, 16, 128, 2); between 2048 rows, 4.3 - 7.6 x, and this nothing is
# measured), and the fp64 MAF of at most two features with 128 or more hidden units (0.89 - 1.05 x at (1024, 2, 128, 2))
LOOP_FROM_ROWS, LOOP_FROM_FEATURES, LOOP_FROM_HIDDEN = 65536, 16, 128


def _masked_layers(made):
    """The MADE's masked linear layers in evaluation order."""
    layers = [made.initial_layer]
    for blk in made.blocks:
        layers += list(blk.linear_layers)
    return layers + [made.final_layer]


def _context_layers(made):
    """The context projections in evaluation order: the MADE's own, then one per block; [] without context."""
    if not hasattr(made, 'context_layer'):
        return []
    return [made.context_layer] + [blk.context_layer for blk in made.blocks]


def _key(made):
    tensors = []
    for lay in _masked_layers(made):
        tensors += [lay.weight, lay.bias, lay.mask, lay.degrees]
    for lay in _context_layers(made):
        tensors += [lay.weight, lay.bias]
    return derived.tensor_key(tensors)


def orders(made):
    """(variable order [D], hidden unit order [H], hidden degrees [H], input degrees [D]) from the module's degree
    buffers, or None where the layers do not share one set of hidden degrees or the input degrees are not 1 .. D."""
    first, final = made.initial_layer, made.final_layer
    d = first.in_features
    if d < 1 or final.out_features % d:
        return None
    in_deg = final.degrees[::final.out_features // d]
    hid_deg = first.degrees
    if in_deg.numel() != d or not torch.equal(torch.sort(in_deg).values, torch.arange(1, d + 1, device=in_deg.device)):
        return None
    for lay in _masked_layers(made)[1:-1]:
        if lay.degrees.shape != hid_deg.shape or not torch.equal(lay.degrees, hid_deg):
            return None
    return torch.argsort(in_deg), torch.argsort(hid_deg, stable=True), hid_deg, in_deg


def _build(made):
    """(wpack, tables, ctx_w [1 + nb, H, C] | None, ctx_b [1 + nb, H] | None), or None for a MADE the stage rule does
    not cover."""
    found = orders(made)
    if found is None:
        return None
    var_order, unit_order, hid_deg, in_deg = found
    layers = _masked_layers(made)
    final = layers[-1]
    d, h = in_deg.numel(), hid_deg.numel()
    mult = final.out_features // d
    out_deg = in_deg.repeat_interleave(mult)
    if not torch.equal(final.degrees, out_deg):
        return None
    rules = [hid_deg[:, None] >= in_deg[None, :]] + [hid_deg[:, None] >= hid_deg[None, :]] * (len(layers) - 2) + \
            [out_deg[:, None] > hid_deg[None, :]]
    for lay, rule in zip(layers, rules):
        if lay.mask.shape != rule.shape or not bool((lay.mask <= rule.to(lay.mask.dtype)).all()):
            return None
    out_rows = (var_order[:, None] * mult + torch.arange(mult, device=var_order.device)[None, :]).reshape(-1)
    parts = []
    for n, lay in enumerate(layers):
        rows = out_rows if lay is final else unit_order
        cols = var_order if n == 0 else unit_order
        parts += [(lay.weight * lay.mask)[rows][:, cols].reshape(-1), lay.bias[rows]]
    wpack = torch.cat(parts).contiguous()
    counts = (hid_deg[None, :] <= torch.arange(d, device=hid_deg.device)[:, None]).sum(1)
    tables = torch.cat([var_order, counts]).to(torch.int32).contiguous()
    ctx = _context_layers(made)
    if not ctx:
        return wpack, tables, None, None
    return (wpack, tables, torch.stack([lay.weight[unit_order] for lay in ctx]).contiguous(),
            torch.stack([lay.bias[unit_order] for lay in ctx]).contiguous())


def pack(made):
    """The kernel's operands for ``made`` (module docstring), kept in the module's ``made_sample`` slot and rewritten in
    place when a parameter or buffer changes; None for a MADE whose masks or degrees the stage rule does not cover."""
    return derived.packed(made, SLOT, _key(made), _build)


def _is_relu(act):
    return act is F.relu or act is torch.relu or isinstance(act, nn.ReLU)


def _records_grad(made, *tensors):
    if not torch.is_grad_enabled():
        return False
    return any(t is not None and t.requires_grad for t in tensors) or any(p.requires_grad for p in made.parameters())


def plan(layer, inputs, context, params_per_feature):
    """The packed operands if ``layer.inverse(inputs, context)`` takes the kernel (module docstring), else None: the
    predicate ``eligible`` and the lookup of the derived buffer in one step, because the layers need both per call.
    The measured ``LOOP_FROM_*`` regions are part of the answer, so a layer changes path - and the last bits of a row -
    where its batch crosses ``LOOP_FROM_ROWS``; the kernel itself gives a row the same bits at every batch."""
    if not getattr(layer, 'fuse_sampling', True) or getattr(layer, 'per_feature', False):
        return None
    made = layer.autoregressive_net
    if type(made) is not MADE or made.preprocessing is not None:
        return None
    if not (torch.is_tensor(inputs) and inputs.is_cuda and inputs.dim() == 2 and inputs.is_contiguous()
            and inputs.dtype in (torch.float32, torch.float64) and inputs.shape[1] == made.initial_layer.in_features
            and inputs.shape[0] > 0):
        return None
    weight = made.initial_layer.weight
    if weight.dtype != inputs.dtype or weight.device != inputs.device:
        return None
    for blk in made.blocks:
        if type(blk) is not MaskedResidualBlock or blk.use_batch_norm or not _is_relu(blk.activation) \
                or (blk.dropout.p > 0 and blk.training):
            return None
    if context is not None:
        if not hasattr(made, 'context_layer') or not (torch.is_tensor(context) and context.dim() == 2
                                                      and context.dtype == inputs.dtype
                                                      and context.device == inputs.device
                                                      and context.shape[0] == inputs.shape[0]
                                                      and context.shape[1] == made.context_layer.in_features):
            return None
    if _records_grad(made, inputs, context):
        return None
    features, hidden = inputs.shape[1], made.initial_layer.out_features
    if hidden >= LOOP_FROM_HIDDEN and ((inputs.shape[0] >= LOOP_FROM_ROWS and features >= LOOP_FROM_FEATURES) or
                                       (inputs.dtype == torch.float64 and params_per_feature == 2 and features <= 2)):
        return None
    if not _lib.made_sample_supported(inputs.shape[1], made.initial_layer.out_features, len(made.blocks),
                                      params_per_feature, inputs.element_size()):
        return None
    return pack(made)


def eligible(layer, inputs, context=None):
    """Whether ``layer.inverse(inputs, context)`` takes the kernel: ``plan`` with the layer's own parameter count, as a
    predicate."""
    return plan(layer, inputs, context, layer._output_dim_multiplier()) is not None


def run(layer, packed, inputs, context, cfg, log_q=None, sign=1.0):
    """One launch of the kernel on ``plan``'s operands: (outputs, log_det), log_det a fresh [B] tensor holding
    ``sign * log|det|`` or ``log_q`` with that added in place.  ``cfg``: the layer's spline constants, None for the
    affine map."""
    wpack, tables, ctx_w, ctx_b = packed
    made = layer.autoregressive_net
    ctx_add = ctx_gate = None
    if context is not None:
        n, b = ctx_w.shape[0], inputs.shape[0]
        # every context projection in one batched GEMM, [1 + nb, B, H]: the MADE's own, then the blocks' gates
        proj = torch.baddbmm(ctx_b[:, None, :], context.detach().expand(n, b, context.shape[1]), ctx_w.transpose(1, 2))
        ctx_add, ctx_gate = proj[0], (proj[1:] if n > 1 else None)
    return _lib.made_sample(inputs.detach(), wpack, tables, ctx_add, ctx_gate, made.initial_layer.out_features,
                            len(made.blocks), made.final_layer.out_features // inputs.shape[1], cfg, logdet=log_q,
                            sign=sign)
