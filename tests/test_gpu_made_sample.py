"""The sampling direction of the autoregressive flows in one launch (csrc/made_sample.hip) on the GPU, against the
reference's loop of D MADE passes (the same layer with ``fuse_sampling = False``).

fp32: the reference is the loop on a ``.double()`` copy, the yardstick the fp32 loop's own error against it; per tensor
``max|kernel - ref64| <= 4 max|loop32 - ref64| + 8 eps32 (1 + max|ref64|)`` (the margin of tests/test_gpu_logit.py).
fp64: nothing more precise than the fp64 loop exists, so the yardstick is the difference between two legitimate
summation orders of the reference - the fp64 loop on the device and oracle.layers' loop on the CPU - and the kernel stays
within 4 x that difference + 1e-13 (1 + max|ref|) of the device loop.  Every figure is printed (``MADESAMPLE`` lines;
profiles/ar_sampling.md holds a run's).

Test layers and inputs: tests/made_sample_ref.py (``init_identity=False``, final layer O(1), the blocks' second linear
layers re-drawn at 1 / sqrt(H); inputs 1.5 randn, with a tail bound of 1.5 in the ``uneven`` spline cases)."""
import copy

import pytest
import torch
from torch.nn import functional as F

import made_sample_ref as R
import vcnf_amd as nf
from vcnf_amd import _lib, made_sample
from vcnf_amd.flows.neural_spline.autoregressive import MaskedPiecewiseRationalQuadraticAutoregressive

pytestmark = pytest.mark.gpu

EPS32 = float(torch.finfo(torch.float32).eps)
CASES = [(kind, name, "linear") for kind in ("affine", "spline") for name in R.STRUCTURES if R.applies(kind, name)] + \
        [("spline", "uneven", tails) for tails in ("circular", "none")]
IDS = ["-".join(c) for c in CASES]
GRID_CAP = 1024                               # kMaxGrid of csrc/made_sample.hip


def layer_for(kind, name, tails, seed=11):
    return R.make_layer(kind, name, seed=seed, tails=R.TAILS[tails], tail_bound=1.5 if name == "uneven" else 3.0)


def tile_of(lay, dtype=torch.float32):
    """Samples a workgroup takes per trip."""
    d, h, nb, p = R.dims(lay)
    lanes = int(nf.lib().vcnf_made_sample_lanes(d, h, nb, p, torch.empty(0, dtype=dtype).element_size()))
    assert lanes in (8, 16, 32, 64)
    return 256 // lanes


def loop_copy(lay, dtype=None):
    other = copy.deepcopy(lay)
    other.fuse_sampling = False
    return other if dtype is None else other.to(dtype)


def takes_kernel(lay, x, ctx, no_grad=True):
    """Whether ``lay.inverse(x, ctx)`` would take the kernel, as the tests call it (under ``torch.no_grad()``)."""
    with torch.set_grad_enabled(not no_grad):
        return made_sample.eligible(lay, x, ctx)


def run(lay, x, ctx):
    with torch.no_grad():
        return lay.inverse(x, ctx) if ctx is not None else lay.inverse(x)


def check_f32(tag, got, loop32, ref64):
    for what, g, l, r in zip(("y", "log_det"), got, loop32, ref64):
        assert g.dtype == torch.float32 and g.shape == r.shape and torch.isfinite(r).all(), what
        err, noise, size = float((g.double() - r).abs().max()), float((l.double() - r).abs().max()), float(r.abs().max())
        print("MADESAMPLE f32 %-34s %-8s max|kernel - ref64| %.3e  max|loop32 - ref64| %.3e  ratio %5.2f  of %.3e"
              % (tag, what, err, noise, err / max(noise, 1e-300), size))
        assert err <= 4 * noise + 8 * EPS32 * (1 + size), "%s %s: %.3e > 4 x %.3e + 8 eps (1 + %.3e)" % (tag, what, err, noise, size)


@pytest.mark.parametrize("kind,name,tails", CASES, ids=IDS)
def test_values_f32(hip, kind, name, tails):
    """The issue's bound, per tensor and per batch (module docstring).  The kernel's sums, logits and inversion are
    double, so its error against the fp64 loop is the rounding of the stored activations and of y (figures:
    profiles/ar_sampling.md)."""
    lay = layer_for(kind, name, tails).to(hip)
    loop32, loop64 = loop_copy(lay), loop_copy(lay, torch.float64)
    tile = tile_of(lay)
    for batch in sorted({1, tile - 1, tile + 1}):
        x, ctx = R.inputs_for(lay, batch, seed=100 + batch)
        x, ctx = x.to(hip), (ctx.to(hip) if ctx is not None else None)
        assert takes_kernel(lay, x, ctx) and not takes_kernel(loop32, x, ctx)
        got = run(lay, x, ctx)
        want32 = run(loop32, x, ctx)
        want64 = run(loop64, x.double(), ctx.double() if ctx is not None else None)
        check_f32("%s B=%d" % ("-".join((kind, name, tails)), batch), got, want32, want64)
    nf.check_discriminant()


@pytest.mark.parametrize("kind,name,tails", CASES, ids=IDS)
def test_values_f64(hip, kind, name, tails):
    lay = layer_for(kind, name, tails).double().to(hip)
    loop = loop_copy(lay)
    tile = tile_of(lay, torch.float64)
    for batch in sorted({1, tile - 1, tile + 1}):
        x, ctx = R.inputs_for(lay, batch, seed=200 + batch, dtype=torch.float64)
        with torch.no_grad():
            cpu = R.oracle_inverse(lay, x, ctx)
        x, ctx = x.to(hip), (ctx.to(hip) if ctx is not None else None)
        assert takes_kernel(lay, x, ctx)
        got, dev = run(lay, x, ctx), run(loop, x, ctx)
        for what, g, d, c in zip(("y", "log_det"), got, dev, cpu):
            assert g.dtype == torch.float64 and torch.isfinite(d).all()
            err, orders, size = float((g - d).abs().max()), float((d.cpu() - c).abs().max()), float(d.abs().max())
            print("MADESAMPLE f64 %-34s %-8s max|kernel - loop| %.3e  max|loop - cpu loop| %.3e  of %.3e"
                  % ("%s B=%d" % ("-".join((kind, name, tails)), batch), what, err, orders, size))
            assert err <= 4 * orders + 1e-13 * (1 + size), "%s: %.3e > 4 x %.3e + 1e-13 (1 + %.3e)" % (what, err, orders, size)
    nf.check_discriminant()


@pytest.mark.parametrize("kind", ["affine", "spline"])
def test_batch_past_the_grid_cap(hip, kind):
    """Two full trips of every workgroup through its tile loop and a ragged third, at the smallest structure
    (the convention of profiles/grid_caps.md)."""
    lay = layer_for(kind, "d1", "linear").to(hip)
    tile = tile_of(lay)
    batch = 2 * GRID_CAP * tile + tile + 1
    x, _ = R.inputs_for(lay, batch, seed=7)
    x = x.to(hip)
    assert takes_kernel(lay, x, None) and -(-batch // tile) > 2 * GRID_CAP
    got = run(lay, x, None)
    check_f32("%s-d1 B=%d" % (kind, batch), got, run(loop_copy(lay), x, None), run(loop_copy(lay, torch.float64), x.double(), None))
    # rows of the second and third trips, as batches of their own: the same bits
    for lo, hi in ((GRID_CAP * tile - 3, GRID_CAP * tile + 5), (2 * GRID_CAP * tile - 1, batch)):
        part = run(lay, x[lo:hi].contiguous(), None)
        assert torch.equal(part[0], got[0][lo:hi]) and torch.equal(part[1], got[1][lo:hi])
    nf.check_discriminant()


ROUND_TRIPS = [("spline", "uneven", torch.float64), ("spline", "permuted", torch.float64), ("spline", "notebook", torch.float64),
               ("affine", "context", torch.float32), ("affine", "context", torch.float64),
               ("affine", "gaps", torch.float32), ("affine", "gaps", torch.float64)]


def round_trip(lay, x, ctx):
    """(z, ld) of the one-pass density direction and (back, ld2) of the sampling direction on that z."""
    with torch.no_grad():
        z, ld = lay.forward(x, ctx)
        z = z.contiguous()
        assert takes_kernel(lay, z, ctx)
        back, ld2 = lay.inverse(z, ctx)
    return z, ld, back, ld2


@pytest.mark.parametrize("kind,name,dtype", ROUND_TRIPS, ids=["%s-%s-%s" % (k, n, str(d)[-7:]) for k, n, d in ROUND_TRIPS])
def test_round_trip_through_the_density_direction(hip, kind, name, dtype):
    """inverse(forward(x)) against x and the two log-dets against 0, under the bounds of test_g19 / test_g22 (mean errors
    below 2e-5 and 1e-4): the MAF layers in both precisions and the spline layers in fp64.  The fp32 spline layers have
    the test below."""
    lay = layer_for(kind, name, "linear").to(hip).to(dtype)
    x, ctx = R.inputs_for(lay, 64, seed=3, dtype=dtype)
    x, ctx = x.to(hip), (ctx.to(hip) if ctx is not None else None)
    z, ld, back, ld2 = round_trip(lay, x, ctx)
    dz, dl = float((back - x).abs().mean()), float((ld + ld2).abs().mean())
    print("MADESAMPLE round trip %s-%s %s  mean|back - x| %.3e  mean|ld + ld2| %.3e" % (kind, name, dtype, dz, dl))
    assert dz < 2e-5 and dl < 1e-4
    nf.check_discriminant()


@pytest.mark.parametrize("name", ["uneven", "permuted", "notebook"])
def test_round_trip_of_the_fp32_spline_layers(hip, name):
    """The fp32 spline layers of this file do not meet test_g19's round-trip bounds with this kernel: mean|ld + ld2| is
    1.05e-4 (``uneven``, tail bound 1.5), 1.51e-4 (``permuted``) and 3.3e-4 (``notebook``) against 1e-4, where the loop has
    5.9e-5, 5.1e-5 and 2.4e-4 (mean|back - x| stays under 2e-5).  The kernel inverts in double, so it returns the preimage
    of the fp32 density pass's ROUNDED z, and the discrepancy is that pass's own rounding; the loop repeats the pass's
    fp32 spline arithmetic and its errors partly cancel.  That claim is what is asserted here, on the same layers and rows:
    (a) the kernel on z32 against the fp64 loop on ``z32.double()`` - the exact preimage - under the value bound of this
        file, ``4 x`` the fp32 loop's own error on z32 ``+ 8 eps (1 + max|ref|)``;
    (b) mean|back - x| and mean|ld + ld2| of the kernel at most twice what that exact preimage itself gives,
        ``+ 8 eps (1 + max|.|)``: the round trip is no worse than the density pass makes it."""
    lay = layer_for("spline", name, "linear").to(hip)
    loop32, loop64 = loop_copy(lay), loop_copy(lay, torch.float64)
    x = R.inputs_for(lay, 64, seed=3)[0].to(hip)
    z, ld, back, ld2 = round_trip(lay, x, None)
    exact = run(loop64, z.double(), None)
    check_f32("round trip %s, on z32" % name, (back, ld2), run(loop32, z, None), exact)
    for what, got, want, size in (("mean|back - x|", (back - x).abs().mean(), (exact[0] - x.double()).abs().mean(), x.abs().max()),
                                  ("mean|ld + ld2|", (ld + ld2).abs().mean(), (ld.double() + exact[1]).abs().mean(), ld.abs().max())):
        print("MADESAMPLE round trip spline-%s fp32  %s kernel %.3e  exact preimage %.3e" % (name, what, float(got), float(want)))
        assert float(got) <= 2 * float(want) + 8 * EPS32 * (1 + float(size)), what
    nf.check_discriminant()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,name", [("spline", "notebook"), ("affine", "context")])
def test_same_bits_twice_and_at_every_batch(hip, kind, name, dtype):
    lay = layer_for(kind, name, "linear").to(hip).to(dtype)
    x, ctx = R.inputs_for(lay, 3 * tile_of(lay, dtype) + 5, seed=9, dtype=dtype)
    x, ctx = x.to(hip), (ctx.to(hip) if ctx is not None else None)
    first, second = run(lay, x, ctx), run(lay, x, ctx)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    # the kernel, unlike the library GEMM, does not choose its algorithm by the batch size.  (The context projections
    # are a library GEMM: that case compares rows of one call's projections, so it runs without context.)
    if ctx is None:
        one = run(lay, x[:1].contiguous(), None)
        assert torch.equal(one[0], first[0][:1]) and torch.equal(one[1], first[1][:1])
        last = run(lay, x[-7:].contiguous(), None)
        assert torch.equal(last[0], first[0][-7:]) and torch.equal(last[1], first[1][-7:])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_direct_call_and_accumulating_form(hip, dtype):
    """``_lib.made_sample`` on the packed operands is what the layer runs, and with a ``logdet`` it adds ``sign * ld``."""
    for kind in ("affine", "spline"):
        lay = layer_for(kind, "uneven", "linear").to(hip).to(dtype)
        x = R.inputs_for(lay, 40, seed=4, dtype=dtype)[0].to(hip)
        d, h, nb, p = R.dims(lay)
        packed = made_sample.pack(lay.autoregressive_net)
        assert packed is not None and packed[0].dtype == dtype and packed[1].dtype == torch.int32
        cfg = lay._spline_cfg() if kind == "spline" else None
        y, ld = _lib.made_sample(x, packed[0], packed[1], None, None, h, nb, p, cfg)
        want = run(lay, x, None)
        assert torch.equal(y, want[0]) and torch.equal(ld, want[1])
        base = torch.linspace(-1, 1, 40, dtype=dtype, device=hip)
        log_q = base.clone()
        y2, out = _lib.made_sample(x, packed[0], packed[1], None, None, h, nb, p, cfg, logdet=log_q, sign=-1.0)
        assert out is log_q and torch.equal(y2, y) and torch.equal(log_q, base - ld)
        log_q = base.clone()
        with torch.no_grad():
            assert torch.equal(lay.inverse_into(x, log_q), y) and torch.equal(log_q, base + ld)
    nf.check_discriminant()


def three_layer_model(hip, dtype=torch.float32):
    torch.manual_seed(21)
    spline = nf.flows.AutoregressiveRationalQuadraticSpline(6, 1, 32, num_bins=8, tail_bound=2.0, init_identity=False)
    maf = nf.flows.MaskedAffineAutoregressive(6, 32, num_blocks=2)
    R.redraw(spline.mprqat.autoregressive_net)
    R.redraw(maf.autoregressive_net)
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(6), [spline, nf.flows.Permute(6, mode="swap"), maf])
    return model.to(dtype).to(hip).eval()


def switched_off(model, dtype=None):
    other = copy.deepcopy(model)
    for m in other.modules():
        if hasattr(m, "fuse_sampling"):
            m.fuse_sampling = False
    return other if dtype is None else other.to(dtype)


def test_through_the_model(hip):
    """sample_from (the spline layer's kernel, log_q folded in the kernel) and log_prob (the MAF's) against the model
    with the switch off, within the fp32 bound."""
    model = three_layer_model(hip)
    loop32, loop64 = switched_off(model), switched_off(model, torch.float64)
    g = torch.Generator().manual_seed(8)
    eps = torch.randn(50, 6, generator=g).to(hip)
    with torch.no_grad():
        got, want32, want64 = model.sample_from(eps), loop32.sample_from(eps), loop64.sample_from(eps.double())
        check_f32("model sample_from", got, want32, want64)
        x = want64[0].float().contiguous()
        lp = (model.log_prob(x), loop32.log_prob(x), loop64.log_prob(x.double()))
        check_f32("model log_prob", lp[:1], lp[1:2], lp[2:])
    nf.check_discriminant()


def test_under_autograd_the_loop_runs_and_trains(hip):
    for kind in ("affine", "spline"):
        lay = layer_for(kind, "uneven", "linear").to(hip)
        x = R.inputs_for(lay, 12, seed=2)[0].to(hip)
        with torch.enable_grad():
            assert all(p.requires_grad for p in lay.parameters()) and not takes_kernel(lay, x, None, no_grad=False)
            y, ld = lay.inverse(x)
            assert y.grad_fn is not None and ld.grad_fn is not None
            (y.sum() + ld.sum()).backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in lay.parameters())
        assert takes_kernel(lay, x, None)
    model = three_layer_model(hip)
    model.train()
    z, log_q = model.sample(16)                     # parameters require grad: every layer takes its differentiable path
    assert log_q.grad_fn is not None


def test_ineligible_layers_give_the_loops_bits(hip):
    torch.manual_seed(5)
    layers = [
        nf.flows.MaskedAffineAutoregressive(6, 32, num_blocks=2, use_residual_blocks=False),
        nf.flows.MaskedAffineAutoregressive(6, 32, num_blocks=1, activation=F.tanh),
        MaskedPiecewiseRationalQuadraticAutoregressive(6, 32, num_bins=8, tails="linear", tail_bound=3.0, num_blocks=1,
                                                       activation=F.tanh, init_identity=False),
        MaskedPiecewiseRationalQuadraticAutoregressive(6, 32, num_bins=8, tails="linear", tail_bound=3.0, num_blocks=2,
                                                       use_residual_blocks=False, init_identity=False),
        # a bin count without a kernel instance (8, 10 and 16 have one)
        MaskedPiecewiseRationalQuadraticAutoregressive(6, 32, num_bins=4, tails="linear", tail_bound=3.0, num_blocks=1,
                                                       init_identity=False),
    ]
    for lay in layers:
        lay = lay.to(hip).eval()
        x = R.inputs_for(lay, 20, seed=6)[0].to(hip)
        assert lay.fuse_sampling and not takes_kernel(lay, x, None)
        got, want = run(lay, x, None), run(loop_copy(lay), x, None)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # eligible layer, ineligible calls: half precision inputs, a non-contiguous view
    lay = layer_for("affine", "uneven", "linear").to(hip)
    x = R.inputs_for(lay, 20, seed=6)[0].to(hip)
    assert takes_kernel(lay, x, None) and not takes_kernel(lay, x.t().contiguous().t(), None) and not takes_kernel(lay, x.half(), None)
    nf.check_discriminant()
