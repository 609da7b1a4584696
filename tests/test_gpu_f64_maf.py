"""``.double()`` masked affine autoregressive flows (MaskedAffineAutoregressive) on vcnf_maf_affine_f64
(csrc/affine_kernels.hip), and a ``.double()`` multiscale Glow: together with tests/test_gpu_f64.py,
tests/test_gpu_f64_grad.py and tests/test_gpu_f64_image.py, every layer family of the library runs in fp64.

Tolerances: layer outputs against the reference's own fp64 outputs (fixtures G22, G11) within 1e-10 (the MADE's and the
conditioners' library GEMMs / convolutions sum in their own order); the kernel against the reference's torch composition
on the same MADE output within 1e-13."""
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib
from helpers import fixture, T, state_for, glow_state
from test_gpu_parity import _glow_model
from test_gpu_f64 import close64

pytestmark = pytest.mark.gpu

F64 = torch.float64


def _maf64(tag):
    fx = fixture("g22_maf")
    lay = (nf.flows.MaskedAffineAutoregressive(7, 24, num_blocks=2) if tag == "plain"
           else nf.flows.MaskedAffineAutoregressive(7, 24, context_features=3, num_blocks=1))
    sd, _ = state_for(fx, tag, 2201, F64, final_gain=1.0)
    for key, v in fx.items():
        if key.startswith(tag + "/mask/"):
            sd[key[len(tag) + 6:]] = T(v, F64)
    lay.load_state_dict(sd)
    return fx, lay.double().cuda().eval()


def _composition(lay, x, params, inverse):
    """The reference's own elementwise map (flows/affine/autoregressive.py:75-89) in torch ops."""
    p = params.view(-1, lay.features, 2)
    scale = torch.sigmoid(p[..., 0] + 2.) + 1e-3
    log_scale = torch.log(scale).sum(1)
    if inverse:
        return (x - p[..., 1]) / scale, -log_scale
    return scale * x + p[..., 1], log_scale


@pytest.mark.parametrize("tag", ["plain", "ctx"])
def test_g22_masked_affine_autoregressive_f64(hip, tag):
    fx, lay = _maf64(tag)
    x = T(fx["x"], F64).cuda()
    kw = {"context": T(fx["ctx"], F64).cuda()} if tag == "ctx" else {}
    with torch.no_grad():
        for dirn, fn in (("fwd", lay.forward), ("inv", lay.inverse)):
            z, ld = fn(x, **kw)
            close64(z, fx["%s/%s_z64" % (tag, dirn)], dirn + " z", rtol=1e-10, atol=1e-10)
            close64(ld, fx["%s/%s_ld64" % (tag, dirn)], dirn + " ld", rtol=1e-10, atol=1e-10)
        z, ld = lay.forward(x, **kw)
        back, ld2 = lay.inverse(z, **kw)
        assert float((back - x).abs().max()) < 1e-12 and float((ld + ld2).abs().max()) < 1e-12
        # the kernel against the reference's composition on the same MADE output, both directions
        params = lay.autoregressive_net(x, kw.get("context"))
        for inverse in (False, True):
            got = _lib.maf_affine(x, params, inverse)
            want = _composition(lay, x, params, inverse)
            for g, w, nm in zip(got, want, ("y", "ld")):
                close64(g, w.cpu().numpy(), "kernel vs composition %s inverse=%s" % (nm, inverse), rtol=1e-13, atol=1e-13)


def test_maf_wrapper_refuses_mixed_dtypes(hip):
    x = torch.randn(5, 7, dtype=F64, device="cuda")
    params = torch.randn(5, 14, dtype=F64, device="cuda")
    y, ld = _lib.maf_affine(x, params, False)
    assert y.dtype == ld.dtype == F64
    with pytest.raises(nf.VcnfError):
        _lib.maf_affine(x, params.float(), False)
    with pytest.raises(nf.VcnfError):
        _lib.maf_affine(x.float(), params, True)


def _maf_flow64(seed=5):
    torch.manual_seed(seed)
    flows = []
    for _ in range(3):
        flows += [nf.flows.MaskedAffineAutoregressive(5, 16, num_blocks=1), nf.flows.Permute(5, mode="swap")]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(5), flows)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.1 * torch.randn_like(p))
    return model.double().cuda()


def test_normalizing_flow_with_maf_layers_f64(hip):
    """log_prob and sample of a .double() NormalizingFlow of MAF layers under no_grad (the HIP kernel) agree with
    the differentiable path (the torch composition)."""
    model = _maf_flow64()
    g = torch.Generator().manual_seed(9)
    x = torch.randn(64, 5, generator=g, dtype=F64).cuda()
    eps = torch.randn(64, 5, generator=g, dtype=F64).cuda()
    with torch.no_grad():
        lp = model.log_prob(x)
        z, lq = model.sample_from(eps)
    assert lp.dtype == z.dtype == lq.dtype == F64
    xg = x.clone().requires_grad_()
    lp_g = model.log_prob(xg)
    eg = eps.clone().requires_grad_()
    z_g, lq_g = model.sample_from(eg)
    close64(lp, lp_g.detach().cpu().numpy(), "log_prob", rtol=1e-12, atol=1e-12)
    close64(z, z_g.detach().cpu().numpy(), "sample z", rtol=1e-12, atol=1e-12)
    close64(lq, lq_g.detach().cpu().numpy(), "sample log_q", rtol=1e-12, atol=1e-12)
    # sampled points are scored back to the density the sampler reports
    with torch.no_grad():
        close64(model.log_prob(z), lq.cpu().numpy(), "log_prob of samples", rtol=1e-10, atol=1e-10)
        zs, lqs = model.sample(7)
    assert zs.shape == (7, 5) and lqs.dtype == F64 and torch.isfinite(lqs).all()


def test_g11_glow_multiscale_f64(hip):
    fx = fixture("g11_glow_multiscale")
    model = _glow_model()
    model.load_state_dict(glow_state(fx, 1101, F64), strict=True)
    model = model.double().cuda().eval()
    with torch.no_grad():
        lp = model.log_prob(T(fx["x"], F64).cuda())
        close64(lp, fx["glow/lp64"], "log_prob", rtol=1e-10, atol=1e-10)
        z, lq = model.sample_from([T(fx["eps0"], F64).cuda(), T(fx["eps1"], F64).cuda()])
        close64(z, fx["glow/s_z64"], "sample z", rtol=1e-10, atol=1e-10)
        close64(lq, fx["glow/s_logq64"], "sample log_q", rtol=1e-10, atol=1e-10)
