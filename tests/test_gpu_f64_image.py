"""``.double()`` image-shaped spline couplings (PiecewiseRationalQuadraticCoupling with img_shape and a ConvResidualNet
conditioner): the fp64 strided spline (vcnf_rqs_elementwise_strided_f64) and its VJP on the conditioner layout
(vcnf_rqs_packed_bwd_f64), csrc/rqs_f64.hip.

Tolerances follow tests/test_gpu_f64.py and tests/test_gpu_f64_grad.py: layer outputs against the reference's own fp64
outputs (fixture G17) within 1e-10 (z) and 1e-9 (log-det); spline gradients against torch autograd over the oracle in
fp64 with every element within 1e-9 of the rms plus 1e-9 of itself; layer gradients within 1e-9 of the rms.  The image
kernels share their device code with the dense fp64 kernels, so on the same logits they must agree bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vcnf_amd as nf
from vcnf_amd import _lib, autograd as vag
from oracle import layers as OL, rqs as orqs
from helpers import fixture, T, state_for, oracle_image_rqs_coupling
from test_gpu_parity import _image_coupling
from test_gpu_f64 import close64
from test_gpu_f64_grad import tight, nd_of

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _g17_64(tag):
    fx = fixture("g17_image_rqs")
    sd, _ = state_for(fx, tag, 1701, F64, final_gain=2.0)
    m = _image_coupling(2 if tag == "ctx" else None)
    m.load_state_dict(sd, strict=True)
    return fx, m.double().cuda().eval()


# ---------------------------------------------------------------- 1. G17 in fp64
@pytest.mark.parametrize("tag", ["noctx", "ctx"])
def test_g17_image_rqs_coupling_f64(hip, tag):
    fx, m = _g17_64(tag)
    x = T(fx["x"], F64).cuda()
    ctx = T(fx["ctx"], F64).cuda() if tag == "ctx" else None
    with torch.no_grad():
        for dirn, fn in (("nsf_fwd", m.forward), ("nsf_inv", m.inverse)):
            z, ld = fn(x, ctx)
            close64(z, fx["%s/%s_z64" % (tag, dirn)], dirn + " z", rtol=1e-10, atol=1e-10)
            close64(ld, fx["%s/%s_ld64" % (tag, dirn)], dirn + " ld", rtol=1e-9, atol=1e-9)
        y, ld1 = m.forward(x, ctx)
        back, ld2 = m.inverse(y, ctx)
        # fp64 round trip: the fp32 test allows 2e-2 at the worst element (steep bins)
        assert float((back - x).abs().max()) < 1e-9 and float((ld1 + ld2).abs().max()) < 1e-9
    nf.check_discriminant()


# ---------------------------------------------------------------- 2. the kernels against the dense fp64 kernels
B, C, INNER = 37, 3, (5, 7)           # 3 885 elements: not a multiple of the 256-thread block; odd inner


def _problem(tails, k, seed=0):
    """x [B, C, 5, 7] and the conditioner-layout logits [B, C*P, 5, 7]; tails: x covers the tails too."""
    g = torch.Generator().manual_seed(seed + 31 * k + (0 if tails is None else len(tails)))
    p = 2 * k + nd_of(tails, k)
    if tails is not None:
        x = (torch.rand(B, C, *INNER, generator=g, dtype=F64) * 2 - 1) * 3.6
    else:
        x = torch.rand(B, C, *INNER, generator=g, dtype=F64) * 0.998 + 0.001
    params = torch.randn(B, C * p, *INNER, generator=g, dtype=F64) * 1.5
    gy = torch.randn(B, C, *INNER, generator=g, dtype=F64)
    gl = torch.randn(B, generator=g, dtype=F64)
    return x, params, gy, gl


def _cfg(tails, k):
    return _lib.make_cfg(k, tails, tail_bound=3.0 if tails else 1.0, wh_scale=0.25)


def _split(params, k):
    """[B, C*P, H, W] -> contiguous [B, C, H, W, P] (the reference's reshape / permute, coupling.py:148-151) and its
    three logit tensors."""
    p = params.reshape(B, C, -1, *INNER).permute(0, 1, 3, 4, 2).contiguous()
    return p, p[..., :k], p[..., k:2 * k], p[..., 2 * k:]


TAILS = ["linear", None, "circular"]
BINS = [2, 8, 10, 16, 23]


@pytest.mark.parametrize("tails", TAILS)
@pytest.mark.parametrize("k", BINS)
@pytest.mark.parametrize("inverse", [False, True])
def test_image_kernel_bitwise_equals_dense_f64(hip, tails, k, inverse):
    x, params, _, _ = (t.cuda() for t in _problem(tails, k))
    cfg = _cfg(tails, k)
    y, lad = _lib.rqs_elementwise_image(x, params, cfg, inverse)
    assert y.dtype == lad.dtype == F64 and y.shape == lad.shape == x.shape
    _, uw, uh, ud = _split(params, k)
    y2, lad2 = _lib.rqs_elementwise(x, uw, uh, ud, cfg, inverse)
    assert torch.isfinite(y).all() and torch.isfinite(lad).all()
    assert torch.equal(y, y2) and torch.equal(lad, lad2)
    if tails is not None:
        out = (x < -3.0) | (x > 3.0)
        assert int(out.sum()) > 100 and torch.equal(y[out], x[out]) and not lad[out].any()
    nf.check_discriminant()


@pytest.mark.parametrize("tails", TAILS)
@pytest.mark.parametrize("k", BINS)
@pytest.mark.parametrize("inverse", [False, True])
def test_image_vjp_f64_vs_oracle_autograd_and_dense(hip, tails, k, inverse):
    x, params, gy, gl = _problem(tails, k)
    cfg = _cfg(tails, k)
    xd, pd = x.cuda().requires_grad_(), params.cuda().requires_grad_()
    y, lad = vag.rqs_packed(xd, pd, cfg, inverse=inverse)
    assert y.dtype == lad.dtype == F64 and lad.shape == (B,)
    gx, gp = torch.autograd.grad([y, lad], [xd, pd], [gy.cuda(), gl.cuda()])
    assert gx.dtype == gp.dtype == F64 and gp.shape == params.shape

    # torch autograd over the oracle in fp64 (CPU)
    xo, po = x.clone().requires_grad_(), params.clone().requires_grad_()
    _, uw, uh, ud = _split(po, k)
    if tails is not None:
        yo, lo = orqs.rq_spline_tails(xo, uw * 0.25, uh * 0.25, ud, inverse=inverse, tails=tails, tail_bound=3.0)
    else:
        yo, lo = orqs.rq_spline(xo, uw * 0.25, uh * 0.25, ud, inverse=inverse)
    assert float((y.detach().cpu() - yo.detach()).abs().max()) <= 1e-10
    want = torch.autograd.grad([yo, lo.sum((1, 2, 3))], [xo, po], [gy, gl])
    what = "tails=%s K=%d inverse=%s" % (tails, k, inverse)
    tight(gx, want[0], "g_x " + what)
    tight(gp, want[1], "g_params " + what)

    # the dense fp64 VJP on the permuted copy: the same device code, bit for bit
    _, uw, uh, ud = _split(params.cuda(), k)
    gle = gl.cuda().view(B, 1, 1, 1).expand(x.shape).contiguous()
    gx2, gw, gh, gd = _lib.rqs_elementwise_bwd(x.cuda(), uw, uh, ud, gy.cuda(), gle, cfg, inverse)
    gp2 = torch.cat([gw, gh, gd], -1).permute(0, 1, 4, 2, 3).reshape(params.shape)
    assert torch.equal(gx, gx2) and torch.equal(gp, gp2), what


def test_image_wrappers_refuse_mixed_dtypes(hip):
    x, params, gy, gl = (t.cuda() for t in _problem("linear", 8))
    cfg = _cfg("linear", 8)
    with pytest.raises(nf.VcnfError):
        _lib.rqs_elementwise_image(x, params.float(), cfg, False)
    with pytest.raises(nf.VcnfError):
        _lib.rqs_elementwise_image(x.float(), params, cfg, True)
    for i in range(4):
        args = [x, params, gy, gl]
        args[i] = args[i].float()
        with pytest.raises(nf.VcnfError):
            _lib.rqs_packed_bwd(*args, cfg, False)


# ---------------------------------------------------------------- 3. a whole fp64 image coupling, with gradients
def _oracle_grads(m, direction, x, ctx, gz, gl):
    """Oracle gradients of <gz, z> + <gl, ld> for the coupling ``m`` (its state in fp64 on the CPU):
    (d x, d ctx, {parameter name: gradient})."""
    sd = {k: (v.detach().cpu().clone().requires_grad_() if v.is_floating_point() else v.detach().cpu())
          for k, v in m.state_dict().items()}
    ora = oracle_image_rqs_coupling(sd)
    xo, co = x.detach().cpu().requires_grad_(), ctx.detach().cpu().requires_grad_()
    z, ld = (ora.nsf_forward if direction == "forward" else ora.nsf_inverse)(xo, co)
    names = [n for n, _ in m.named_parameters()]
    g = torch.autograd.grad([z, ld.reshape(-1)], [xo, co] + [sd[n] for n in names], [gz, gl], allow_unused=True)
    return g[0], g[1], dict(zip(names, g[2:]))


@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_image_coupling_f64_layer_gradients_vs_oracle(hip, direction):
    fx, m = _g17_64("ctx")
    x = T(fx["x"], F64).cuda().requires_grad_()
    ctx = T(fx["ctx"], F64).cuda().requires_grad_()
    z, ld = getattr(m, direction)(x, ctx)
    assert z.dtype == ld.dtype == F64
    g = torch.Generator().manual_seed(17)
    gz, gl = torch.randn(z.shape, generator=g, dtype=F64), torch.randn(ld.shape, generator=g, dtype=F64)
    torch.autograd.backward([z, ld], [gz.cuda(), gl.cuda()])
    want_x, want_c, want_p = _oracle_grads(m, direction, x, ctx, gz, gl)
    tight(x.grad, want_x, direction + " input", rel=0.0)
    tight(ctx.grad, want_c, direction + " context", rel=0.0)
    for n, p in m.named_parameters():
        if want_p[n] is None:
            assert p.grad is None or not p.grad.any(), n
            continue
        tight(p.grad, want_p[n], "%s %s" % (direction, n), rel=0.0)


# ---------------------------------------------------------------- 4. training a small fp64 image NSF
LAYERS = 3


def _image_nsf64(seed=21):
    torch.manual_seed(seed)
    net = lambda i, o: nf.nets.ConvResidualNet(in_channels=i, out_channels=o, hidden_channels=16, context_channels=None,
                                               num_blocks=1, activation=F.relu, dropout_probability=0.0,
                                               use_batch_norm=False)
    flows = [nf.flows.neural_spline.coupling.PiecewiseRationalQuadraticCoupling(
        mask=nf.utils.masks.create_alternating_binary_mask(6, even=(i % 2 == 0)), transform_net_create_fn=net,
        num_bins=8, tails="linear", tail_bound=3.0, apply_unconditional_transform=True, img_shape=[8, 8])
        for i in range(LAYERS)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian((6, 8, 8)), flows)
    with torch.no_grad():                  # away from the identity initialisation: every parameter matters
        for p in model.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return model.double().cuda()


def _images(n=256, seed=4):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, 6, 8, 8, generator=g, dtype=F64)
    return torch.cat([a[:, :3], a[:, 3:] * 0.5 + torch.tanh(2 * a[:, :3])], 1) * 0.8 + 0.3


def _oracle_log_prob(sd, x):
    """NormalizingFlow.log_prob over the raw couplings: each layer's ``inverse`` (the coupling's sampling
    direction) from the last to the first, then the Gaussian base."""
    z, log_q = x, 0.0
    for i in reversed(range(LAYERS)):
        pre = "flows.%d." % i
        ora = oracle_image_rqs_coupling({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
        z, ld = ora.nsf_inverse(z)
        log_q = log_q + ld.reshape(-1)
    return log_q + OL.DiagGaussian(sd["q0.loc"], sd["q0.log_scale"]).log_prob(z)


def test_image_nsf_f64_first_adam_step_gradients_vs_oracle(hip):
    model = _image_nsf64()
    x = _images()
    sd = {k: (v.detach().cpu().clone().requires_grad_() if v.is_floating_point() else v.detach().cpu())
          for k, v in model.state_dict().items()}
    want_loss = -_oracle_log_prob(sd, x).mean()
    names = [n for n, _ in model.named_parameters()]
    want = torch.autograd.grad(want_loss, [sd[n] for n in names], allow_unused=True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = model.forward_kld(x.cuda())
    assert loss.dtype == F64
    loss.backward()
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-10 * max(1.0, abs(float(want_loss.detach())))
    params = dict(model.named_parameters())
    for n, w in zip(names, want):
        if w is None:
            assert params[n].grad is None or not params[n].grad.any(), n
            continue
        assert params[n].grad is not None, n
        tight(params[n].grad, w, "image nsf64 " + n, rel=0.0)
    opt.step()


def test_image_nsf_f64_trains(hip):
    model = _image_nsf64()
    x = _images().cuda()
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = model.forward_kld(x)
        assert loss.dtype == F64
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    assert np.isfinite(losses).all() and losses[-1] < losses[0] - 0.1, losses
