"""Training of ``.double()`` spline models: the fp64 spline VJP kernel (vcnf_rqs_elementwise_bwd_f64, csrc/rqs_f64.hip)
and the layers / functional API that route through it, against torch autograd over the oracle in fp64 and against the
reference's own fp64 autograd gradients (fixture G23).

Tolerance: both sides are fp64 and the backward selects the bin of the fp64 forward kernel (shared knot code), so no
element may sit in another bin than the oracle's.  Spline gradients: |got - want| <= 1e-9 rms(want) + 1e-9 |want| for
EVERY element; layer / stack gradients: 1e-9 of the rms (the bound the CPU oracle meets on G23)."""
import numpy as np
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib, autograd as vag
from vcnf_amd.utils import splines
from oracle import layers as OL, nets as ON, rqs as orqs
from helpers import fixture, T, state_for, oracle_crqs_stack, g23_cases, g23_reference
from test_gpu_grad import _g23_build, close as close32

pytestmark = pytest.mark.gpu


def tight(got, want, what, rel=1e-9, rms_frac=1e-9):
    """Every element within rms_frac * rms(want) + rel * |want|."""
    got = got.detach().cpu()
    want = want.detach().cpu()
    assert got.dtype == torch.float64, what + ": result is not fp64"
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what + ": non-finite gradient"
    rms = float(want.pow(2).mean().sqrt())
    err = (got - want).abs()
    bound = rms_frac * rms + rel * want.abs()
    worst = int((err - bound).argmax())
    assert bool((err <= bound).all()), "%s: %d / %d outside, max err %.3e (rms %.3e), worst %.3e vs %.3e" % (
        what, int((err > bound).sum()), err.numel(), float(err.max()), rms, float(err.reshape(-1)[worst]),
        float(want.reshape(-1)[worst]))


def nd_of(tails, k):
    return k - 1 if tails == "linear" else k if tails == "circular" else k + 1


def _spline_problem(tails, k, n=20000, bound=3.0, seed=0):
    g = torch.Generator().manual_seed(seed + 100 + k)
    if tails is not None:
        x = (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * bound * 1.2      # includes the tails
    else:
        x = torch.rand(n, generator=g, dtype=torch.float64) * 0.998 + 0.001
    uw, uh, ud = (torch.randn(n, m, generator=g, dtype=torch.float64) * 1.5 for m in (k, k, nd_of(tails, k)))
    gy, gl = torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)
    return x, uw, uh, ud, gy, gl


def _oracle_spline(x, uw, uh, ud, gy, gl, tails, inverse, bound=3.0):
    leaves = [t.clone().requires_grad_() for t in (x, uw, uh, ud)]
    if tails is not None:
        y, lad = orqs.rq_spline_tails(*leaves, inverse=inverse, tails=tails, tail_bound=bound)
    else:
        y, lad = orqs.rq_spline(*leaves, inverse=inverse)
    return y.detach(), lad.detach(), torch.autograd.grad([y, lad], leaves, [gy, gl])


# ---------------------------------------------------------------- 1. the kernel against oracle autograd
@pytest.mark.parametrize("tails", ["linear", None, "circular"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("k", [5, 8, 10, 16, 23])
def test_f64_spline_vjp_vs_oracle_autograd(hip, tails, inverse, k):
    bound = 3.0
    x, uw, uh, ud, gy, gl = _spline_problem(tails, k, bound=bound)
    y, lad, want = _oracle_spline(x, uw, uh, ud, gy, gl, tails, inverse, bound)
    cfg = _lib.make_cfg(k, tails, tail_bound=bound if tails else 1.0)
    dl = [t.cuda().requires_grad_() for t in (x, uw, uh, ud)]
    yy, ll = vag.rqs_spline(*dl, cfg, inverse=inverse)
    assert yy.dtype == torch.float64
    assert float((yy.detach().cpu() - y).abs().max()) <= 1e-10
    got = torch.autograd.grad([yy, ll], dl, [gy.cuda(), gl.cuda()])
    what = "tails=%s inverse=%s K=%d" % (tails, inverse, k)
    for a, b, nm in zip(got, want, ("g_x", "g_uw", "g_uh", "g_ud")):
        tight(a, b, "%s %s" % (nm, what))
    if tails is not None:
        out = (x < -bound) | (x > bound)
        assert int(out.sum()) > 1000
        gx, gw, gh, gd = (t.cpu() for t in got)
        assert torch.equal(gx[out], gy[out])
        assert not gw[out].any() and not gh[out].any() and not gd[out].any()


def test_f64_vjp_wrapper_checks_dtypes(hip):
    cfg = _lib.make_cfg(8, "linear", tail_bound=3.0)
    x, uw, uh, ud, gy, gl = (t.cuda() for t in _spline_problem("linear", 8, n=64))
    gx, gw, gh, gd = _lib.rqs_elementwise_bwd(x, uw, uh, ud, gy, gl, cfg, False)
    assert gx.dtype == gw.dtype == gd.dtype == torch.float64 and gd.shape == ud.shape
    with pytest.raises(nf.VcnfError):
        _lib.rqs_elementwise_bwd(x, uw.float(), uh, ud, gy, gl, cfg, False)
    with pytest.raises(nf.VcnfError):
        _lib.rqs_elementwise_bwd(x, uw, uh, ud, gy.float(), gl, cfg, False)


# ---------------------------------------------------------------- 2. G23 against the reference's own fp64 autograd
_RQS_CASES = ["layer/forward", "layer/inverse", "c3/log_prob", "c3/sample"]


@pytest.mark.parametrize("tag", _RQS_CASES)
def test_g23_f64_hip_gradients_vs_reference_fp64_autograd(hip, tag):
    """The fixture's "64" gradients are the reference's autograd of its model loaded with the fp32 state and converted
    with .double() (tests/golden/make_golden.py::g23_gradients); the same here on the fp64 HIP path."""
    fx = fixture("g23_gradients")
    case = [c for c in g23_cases() if c[0] == tag][0]
    _, seed, gains, in_names, gz_name, _, _ = case
    sd, _ = state_for(fx, tag, seed, **gains)
    model, loss_fn = _g23_build(tag, fx)
    model.load_state_dict(sd)
    model = model.double().to("cuda").train()
    names, ref = g23_reference(fx, tag, len(in_names))
    xs = [T(fx[n], torch.float64).cuda().requires_grad_() for n in in_names]
    gz = T(fx[gz_name], torch.float64).cuda() if gz_name else None
    val = loss_fn(model, *xs, gz)
    assert val.dtype == torch.float64
    val.backward()
    loss64 = ref["64"][0]
    assert abs(float(val.detach()) - loss64) <= 1e-12 * max(1.0, abs(loss64)), (float(val.detach()), loss64)
    params = dict(model.named_parameters())
    for i, xg in enumerate(xs):
        tight(xg.grad, ref["64"][1][i], "%s input%d" % (tag, i), rel=0.0)
    for n in names:
        assert params[n].grad is not None, n
        tight(params[n].grad, ref["64"][2][n], "%s %s" % (tag, n), rel=0.0)


# ---------------------------------------------------------------- 3. autoregressive RQS in fp64 (G19)
def _ar_layer64(fx, tag):
    if tag == "plain":
        lay = nf.flows.AutoregressiveRationalQuadraticSpline(6, 1, 32, num_bins=8, tail_bound=3.0, init_identity=False)
    else:
        lay = nf.flows.CircularAutoregressiveRationalQuadraticSpline(
            6, 1, 32, ind_circ=[1, 4], num_bins=8, tail_bound=torch.tensor([3.0, float(np.pi), 3.0, 2.5, float(np.pi), 3.0]),
            permute_mask=True, init_identity=False)
    sd, _ = state_for(fx, tag, 1901, torch.float64, final_gain=2.0)      # the fixture's fp64 weights
    for key, v in fx.items():
        if key.startswith(tag + "/mask/"):
            sd[key[len(tag) + 6:]] = T(v, torch.float64)
    lay = lay.double()
    missing = lay.load_state_dict(sd, strict=False).missing_keys
    assert all(("tail_bound" in m) or m.endswith("preprocessing.scale") for m in missing), missing
    return lay.cuda()


def _oracle_ar(sd, tag):
    pre = "mprqat.autoregressive_net."
    if tag == "plain":
        return OL.AutoregressiveRQS(lambda x: ON.made(sd, pre, x), 6, 8, "linear", 3.0)
    # the layer's bounds and periodic scale are fp32 tensors converted by .double() (as in the fixture's fp64 run)
    bound = torch.tensor([3.0, float(np.pi), 3.0, 2.5, float(np.pi), 3.0])
    tails = ["circular" if i in (1, 4) else "linear" for i in range(6)]
    scale = (np.pi / bound[[1, 4]]).double()
    pp = lambda x: ON.periodic_features(sd, pre + "preprocessing.", x, scale)
    return OL.AutoregressiveRQS(lambda x: ON.made(sd, pre, x, preprocess=pp), 6, 8, tails, bound.double())


@pytest.mark.parametrize("tag", ["plain", "circular"])
def test_g19_autoregressive_rqs_f64(hip, tag):
    fx = fixture("g19_autoregressive")
    lay = _ar_layer64(fx, tag)
    x = T(fx["x"], torch.float64).cuda()
    with torch.no_grad():
        for dirn, fn in (("fwd", lay.forward), ("inv", lay.inverse)):
            z, ld = fn(x)
            assert z.dtype == torch.float64
            assert float((z.cpu() - T(fx["%s/%s_z64" % (tag, dirn)])).abs().max()) <= 1e-10, dirn
            assert float((ld.cpu() - T(fx["%s/%s_ld64" % (tag, dirn)])).abs().max()) <= 1e-9, dirn
    # density direction (the wrapper's inverse is the MADE layer's one-pass forward) against oracle autograd
    sd = {k: v.detach().cpu().clone() for k, v in lay.state_dict().items()}
    names = [n for n, _ in lay.named_parameters()]
    for n in names:
        sd[n].requires_grad_()
    ora = _oracle_ar(sd, tag)
    xo = T(fx["x"], torch.float64).requires_grad_()
    g = torch.Generator().manual_seed(19)
    gz = torch.randn(xo.shape, generator=g, dtype=torch.float64)
    z, ld = ora.nsf_forward(xo)
    want = torch.autograd.grad(ld.sum() + (z * gz).sum(), [xo] + [sd[n] for n in names])
    xg = x.clone().requires_grad_()
    z2, ld2 = lay.inverse(xg)
    (ld2.sum() + (z2 * gz.cuda()).sum()).backward()
    tight(xg.grad, want[0], tag + " input")
    params = dict(lay.named_parameters())
    for n, w in zip(names, want[1:]):
        tight(params[n].grad, w, "%s %s" % (tag, n))


# ---------------------------------------------------------------- 4. the functional API is differentiable
@pytest.mark.parametrize("form", ["linear", "circular", "bounded"])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_functional_spline_api_is_differentiable(hip, form, inverse, dtype):
    k, bound = 10, 2.5
    tails = None if form == "bounded" else form
    x, uw, uh, ud, gy, gl = _spline_problem(tails, k, n=8192, bound=bound, seed=7)
    x, uw, uh, ud = (t.reshape(1024, 8, *t.shape[1:]) for t in (x, uw, uh, ud))
    gy, gl = gy.reshape(1024, 8), gl.reshape(1024, 8)
    y, lad, want = _oracle_spline(x, uw, uh, ud, gy, gl, tails, inverse, bound)
    dl = [t.to(dtype).cuda().requires_grad_() for t in (x, uw, uh, ud)]
    if tails is None:
        yy, ll = splines.rational_quadratic_spline(*dl, inverse=inverse)
    else:
        yy, ll = splines.unconstrained_rational_quadratic_spline(*dl, inverse=inverse, tails=tails, tail_bound=bound)
    assert yy.requires_grad and ll.requires_grad
    got = torch.autograd.grad([yy, ll], dl, [gy.to(dtype).cuda(), gl.to(dtype).cuda()])
    what = "%s inverse=%s %s" % (form, inverse, dtype)
    for a, b, nm in zip(got, want, ("g_x", "g_uw", "g_uh", "g_ud")):
        if dtype == torch.float64:
            tight(a, b, "%s %s" % (nm, what))
        else:
            close32(a, b, "%s %s" % (nm, what))


def test_functional_per_feature_list_is_differentiable_f64(hip):
    k, bound, d = 8, 3.0, 6
    tails = ["linear", "circular", "linear", "linear", "circular", "linear"]
    g = torch.Generator().manual_seed(23)
    x = (torch.rand(2048, d, generator=g, dtype=torch.float64) * 2 - 1) * bound * 0.999   # the oracle's list form
    # leaves elements outside the bound unset (its restatement of splines.py:50-57); inside, both are the spline
    uw, uh, ud = (torch.randn(2048, d, m, generator=g, dtype=torch.float64) * 1.5 for m in (k, k, k + 1))
    gy, gl = torch.randn(2048, d, generator=g, dtype=torch.float64), torch.randn(2048, d, generator=g, dtype=torch.float64)
    for inverse in (False, True):
        leaves = [t.clone().requires_grad_() for t in (x, uw, uh, ud)]
        y, lad = orqs.rq_spline_tails(*leaves, inverse=inverse, tails=tails, tail_bound=bound)
        want = torch.autograd.grad([y, lad], leaves, [gy, gl])
        dl = [t.cuda().requires_grad_() for t in (x, uw, uh, ud)]
        yy, ll = splines.unconstrained_rational_quadratic_spline(*dl, inverse=inverse, tails=tails, tail_bound=bound)
        assert float((yy.detach().cpu() - y.detach()).abs().max()) <= 1e-10
        got = torch.autograd.grad([yy, ll], dl, [gy.cuda(), gl.cuda()])
        for a, b, nm in zip(got, want, ("g_x", "g_uw", "g_uh", "g_ud")):
            tight(a, b, "per-feature %s inverse=%s" % (nm, inverse))


def test_plain_wrapper_still_refuses_grad_f64(hip):
    cfg = _lib.make_cfg(8, "linear", tail_bound=3.0)
    x, uw, uh, ud, _, _ = (t.cuda() for t in _spline_problem("linear", 8, n=64))
    with pytest.raises(NotImplementedError):
        _lib.rqs_elementwise(x, uw.requires_grad_(), uh, ud, cfg, False)


# ---------------------------------------------------------------- 5. fp64 training end to end
def _nsf64(seed=11):
    torch.manual_seed(seed)
    flows = [nf.flows.CoupledRationalQuadraticSpline(6, 2, 32, num_bins=10, reverse_mask=bool(i % 2)) for i in range(4)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(6), flows)
    with torch.no_grad():                  # away from the identity initialisation: every parameter matters
        for p in model.parameters():
            p.add_(0.2 * torch.randn_like(p))
    return model.double().cuda()


def _data(n=2048, seed=3):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(n, 6, generator=g, dtype=torch.float64)
    return torch.cat([a[:, :3], a[:, 3:] * 0.5 + torch.tanh(2 * a[:, :3])], 1) * 0.8 + 0.3


def test_f64_nsf_first_adam_step_gradients_vs_oracle(hip):
    model = _nsf64()
    x = _data()
    sd = {k: (v.detach().cpu().clone().requires_grad_() if v.is_floating_point() else v.detach().cpu())
          for k, v in model.state_dict().items()}
    ora = oracle_crqs_stack(sd, 4, 10, 3.0, 32)
    want_loss = -ora.log_prob(x).mean()
    names = [n for n, _ in model.named_parameters()]
    want = torch.autograd.grad(want_loss, [sd[n] for n in names], allow_unused=True)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = model.forward_kld(x.cuda())
    loss.backward()
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-12 * max(1.0, abs(float(want_loss.detach())))
    params = dict(model.named_parameters())
    for n, w in zip(names, want):
        if w is None:
            assert params[n].grad is None or not params[n].grad.any(), n
            continue
        assert params[n].grad is not None, n
        tight(params[n].grad, w, "nsf64 " + n, rel=0.0)
    opt.step()


def test_f64_nsf_trains(hip):
    model = _nsf64()
    x = _data().cuda()
    opt = torch.optim.Adam(model.parameters(), lr=3e-3)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = model.forward_kld(x)
        assert loss.dtype == torch.float64
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    # 30 steps at lr 3e-3 on 2048 samples: the negative log-likelihood falls by at least 0.3 nats
    assert np.isfinite(losses).all() and losses[-1] < losses[0] - 0.3, losses
