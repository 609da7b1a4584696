"""The stage rule and the packing of the one-launch sampling kernel (csrc/made_sample.hip), without a GPU:
tests/made_sample_ref.py restates the staged algorithm in plain torch over the buffers vcnf_amd.made_sample.pack
writes, and here it is compared with oracle.layers' own D-pass loops on the same state dict, in fp64, at every
structure the kernel's tests run.  Both sides are fp64 and differ in the order of their sums only."""
import pytest
import torch
from torch.nn import functional as F

import made_sample_ref as R
from vcnf_amd import made_sample

CASES = [(kind, name, "linear") for kind in ("affine", "spline") for name in R.STRUCTURES if R.applies(kind, name)] + \
        [("spline", "uneven", tails) for tails in ("circular", "none")]


oracle_inverse = R.oracle_inverse


@pytest.mark.parametrize("kind,name,tails", CASES, ids=["-".join(c) for c in CASES])
def test_staged_algorithm_matches_the_loop(kind, name, tails):
    lay = R.make_layer(kind, name, seed=11, tails=R.TAILS[tails], tail_bound=1.5 if name == "uneven" else 3.0).double()
    x, ctx = R.inputs_for(lay, 37, seed=5, dtype=torch.float64)
    with torch.no_grad():
        want_y, want_ld = oracle_inverse(lay, x, ctx)
        got_y, got_ld = R.staged_sample(lay, x, ctx)
    for what, got, want in (("y", got_y, want_y), ("log_det", got_ld, want_ld)):
        assert torch.isfinite(want).all(), what
        excess = ((got - want).abs() - 1e-12 * (1 + want.abs())).max()
        assert float(excess) <= 0, "%s: %.3e over 1e-12 (1 + |ref|)" % (what, float(excess))
    if tails == "linear" and kind == "spline" and name == "uneven":
        outside = float((x.abs() > 1.5).double().mean())
        assert 0.2 < outside < 0.5, outside          # a good share of the elements lies in the linear tails


@pytest.mark.parametrize("name", list(R.STRUCTURES))
def test_packing_and_unpacking_reproduces_the_masked_layers(name):
    lay = R.make_layer("spline", name, seed=3).double()
    made = lay.autoregressive_net
    packed = made_sample.pack(made)
    assert packed is not None
    d, h, nb, p = R.dims(lay)
    assert packed[0].numel() == h * d + h + nb * (2 * h * h + 2 * h) + d * p * h + d * p
    order, count = packed[1][:d], packed[1][d:]
    in_deg = made.final_layer.degrees[::p]
    assert torch.equal(in_deg[order.long()], torch.arange(1, d + 1))
    assert torch.equal(count.long(), torch.stack([(made.initial_layer.degrees <= i).sum() for i in range(d)]))
    torch.manual_seed(0)
    for key, (w, b) in R.unpack(packed, made).items():
        layer = made.get_submodule(key)
        assert torch.equal(w, layer.weight * layer.mask) and torch.equal(b, layer.bias), key
        v = torch.randn(5, layer.in_features, dtype=torch.float64)
        assert torch.equal(F.linear(v, w, b), F.linear(v, layer.weight * layer.mask, layer.bias)), key
    # the slot is rewritten in place when a parameter changes, and forgotten keys rebuild it
    with torch.no_grad():
        made.final_layer.bias.add_(1.0)
    again = made_sample.pack(made)
    assert again[0].data_ptr() == packed[0].data_ptr()
    assert torch.equal(R.unpack(again, made)["final_layer"][1], made.final_layer.bias)


def test_pack_refuses_a_mask_outside_the_degree_rule():
    lay = R.make_layer("spline", "uneven", seed=3).double()
    made = lay.autoregressive_net
    assert made_sample.pack(made) is not None
    mask = made.blocks[0].linear_layers[1].mask
    low, high = int(made.initial_layer.degrees.argmin()), int(made.initial_layer.degrees.argmax())
    assert mask[low, high] == 0
    mask[low, high] = 1.0                       # a unit of the lowest degree sees one of the highest
    assert made_sample.pack(made) is None
    mask[low, high] = 0.0
    assert made_sample.pack(made) is not None
    made.final_layer.mask[0, :] = 1.0           # an output row that sees every hidden unit
    assert made_sample.pack(made) is None


def test_pack_allows_a_mask_stricter_than_the_degree_rule():
    lay = R.make_layer("affine", "uneven", seed=3).double()
    made = lay.autoregressive_net
    made.blocks[0].linear_layers[0].mask[:, 0] = 0.0
    x, _ = R.inputs_for(lay, 9, dtype=torch.float64)
    with torch.no_grad():
        want_y, want_ld = oracle_inverse(lay, x, None)
        got_y, got_ld = R.staged_sample(lay, x)
    assert float((got_y - want_y).abs().max()) < 1e-12 and float((got_ld - want_ld).abs().max()) < 1e-12
