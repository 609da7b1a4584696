"""Derived buffers (vcnf_amd.derived) on the device, through every path that keeps one: after the parameters change the
next evaluation computes, bit for bit, what a newly built model with those parameters computes, from buffers at the
addresses they had before; and no module keeps a device tensor outside the module's containers."""
import pytest
import torch
from torch import nn

import vcnf_amd as nf
from vcnf_amd import derived

B = 33          # one full 32-sample tile and a ragged one


def _flow(dim, flows):
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(dim), flows)


def _rqs(precision):
    def make():
        model = _flow(32, [nf.flows.CoupledRationalQuadraticSpline(32, 1, 128, 8) for _ in range(2)])
        for f in model.flows:
            f.prqct.fused_precision = precision
        return model
    return make


def _affine():
    flows = []
    for _ in range(2):
        flows += [nf.flows.AffineCouplingBlock(nf.nets.MLP([16, 64, 64, 32])), nf.flows.Permute(32, "swap")]
    return _flow(32, flows)


# (model, input shape, the slots the first evaluations must have filled: the test fails when a path was not taken).
# Conditioners are built with random last layers (init_zeros=False) so that scaling every parameter changes the result.
MODELS = {
    "rqs_fp16x3": (_rqs("fp16x3"), (32,), {"rqs_f16x3", "rqs_f32"}),            # (range-safe: the fp32 pack rides along)
    "rqs_fp32": (_rqs("fp32"), (32,), {"rqs_f32"}),
    "affine_stack": (_affine, (32,), {"affine", "affine_run"}),
    # tests/test_gpu_parity.py::test_glow_block_fused_mixers_match_layerwise's block: composed mixer + packed 1x1 convolution
    "glow": (lambda: _flow((24, 8, 8), [nf.flows.GlowBlock(24, 32, init_zeros=False)]), (24, 8, 8),
             {"mixer_density", "conv1x1"}),
    # 256 hidden channels: all three convolutions of the conditioner on the fused kernels
    "glow_convnet3": (lambda: _flow((8, 8, 8), [nf.flows.GlowBlock(8, 256, init_zeros=False)]), (8, 8, 8),
                      {"mixer_density", "conv3x3", "conv1x1", "taps"}),
    # test_final_layer_fused_with_splines' smallest layer (d_t = 21); test_resnet_trunk_kernel_vs_torch's (16 inputs, 1 block)
    "final": (lambda: _flow(42, [nf.flows.CoupledRationalQuadraticSpline(42, 1, 128, 8)]), (42,), {"final"}),
    "final_trunk": (lambda: _flow(32, [nf.flows.CoupledRationalQuadraticSpline(32, 1, 128, 16)]), (32,), {"final", "trunk"}),
    "lu_linear": (lambda: _flow(8, [nf.flows.LULinearPermute(8)]), (8,), set()),                # memos only
}

# attributes that may hold a device tensor outside the containers: none of them derived from parameters
ALLOWED = set()             # (module type name, attribute); nothing in these models needs it
_TORCH_OWN = {"_parameters", "_buffers", "_modules", "_non_persistent_buffers_set", "_backward_hooks", "_backward_pre_hooks",
              "_forward_hooks", "_forward_hooks_with_kwargs", "_forward_hooks_always_called", "_forward_pre_hooks",
              "_forward_pre_hooks_with_kwargs", "_state_dict_hooks", "_state_dict_pre_hooks", "_load_state_dict_pre_hooks",
              "_load_state_dict_post_hooks", "_is_full_backward_hook"}


def _device_tensors(value, depth=0):
    """Device tensors reachable from ``value`` through dicts, lists, tuples and sets (modules are walked on their own)."""
    if torch.is_tensor(value):
        return [value] if value.is_cuda else []
    if isinstance(value, nn.Module) or depth > 6:
        return []
    if isinstance(value, dict):
        value = list(value.keys()) + list(value.values())
    if isinstance(value, (list, tuple, set, frozenset)):
        return [t for v in value for t in _device_tensors(v, depth + 1)]
    return []


def private_device_tensors(model, skip=derived.CONTAINERS):
    """(module type, attribute) of every module attribute outside ``skip``, torch's own dicts and ALLOWED that holds a
    device tensor."""
    found = []
    for m in model.modules():
        for name, value in m.__dict__.items():
            if name in skip or name in _TORCH_OWN or (type(m).__name__, name) in ALLOWED:
                continue
            if _device_tensors(value):
                found.append((type(m).__name__, name))
    return found


def _twin(make, model):
    twin = make().cuda().eval()
    twin.load_state_dict(model.state_dict())
    return twin


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_derived_buffers_follow_the_parameters_in_place(hip, name):
    make, shape, slots = MODELS[name]
    torch.manual_seed(7)
    model = make().cuda().eval()
    x = torch.randn(B, *shape, device="cuda")
    with torch.no_grad():
        model.log_prob(x)                       # (a GlowBlock's ActNorm takes its statistics from the first batch)
        first = model.log_prob(x)
        where = [(m, slot, t, t.data_ptr()) for m, slot, t in derived.buffers(model)]
        assert {slot for _, slot, _, _ in where} == slots, "the path under test was not taken"
        assert torch.equal(first, _twin(make, model).log_prob(x))

        for p in model.parameters():
            p.mul_(1.01)                        # in place, bumps _version: seen by the keys
        second = model.log_prob(x)
        assert torch.isfinite(second).all() and not torch.equal(second, first)
        assert torch.equal(second, _twin(make, model).log_prob(x))
        now = [(m, slot, t, t.data_ptr()) for m, slot, t in derived.buffers(model)]
        assert len(now) == len(where) and all(a[0] is b[0] and a[1] == b[1] and a[2] is b[2] and a[3] == b[3]
                                              for a, b in zip(where, now)), "a buffer moved"

        for p in model.parameters():
            p.data.mul_(1.01)                   # behind the keys' back: needs refresh_packed
        nf.refresh_packed(model)
        third = model.log_prob(x)
        assert torch.isfinite(third).all() and not torch.equal(third, second)
        assert torch.equal(third, _twin(make, model).log_prob(x))
        now = [(m, slot, t, t.data_ptr()) for m, slot, t in derived.buffers(model)]
        assert len(now) == len(where) and all(a[0] is b[0] and a[1] == b[1] and a[2] is b[2] and a[3] == b[3]
                                              for a, b in zip(where, now)), "a buffer moved after refresh_packed"
        model.sample(B)                         # the other direction fills its own slots and memos before the sweep
    assert private_device_tensors(model) == []
