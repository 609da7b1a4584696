"""The flow VAE's end caps without a GPU: the vcnf_vae_* symbols are exported and bound from the header, their host-side
validation returns the documented status codes in the documented order before anything is launched, the plain-torch
restatement the GPU tests compare against (vae_ref.py) is pinned in fp64 to independent implementations, the modules
carry the stated names and shapes, and on CPU tensors a whole NormalizingFlowVAE is the restatement's container."""
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import vae_ref as ref
import vcnf_amd as nf
from helpers import assert_close
from vcnf_amd import _lib

KERNELS = ("encode", "encode_bwd", "gauss_log_prob", "gauss_log_prob_bwd", "bernoulli_log_prob", "bernoulli_log_prob_bwd")
FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / empty batch
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
PIN = dict(rtol=1e-10, atol=1e-10)
OVER = 4097


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    names = ["vcnf_vae_%s%s" % (k, sfx) for k in KERNELS for sfx in ("_f32", "_f64")]
    assert len(names) == 12
    for name in names:
        assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
        assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    assert _lib.VAE_MAX_SAMPLES == 4096 and _lib._ABI.constants["VCNF_VAE_MAX_SAMPLES"] == 4096


def _calls(L, sfx):
    """Per entry point (function (first pointer, rows or batch, divisor, D) -> status with every other pointer valid,
    whether the divisor is limited)."""
    f = lambda k: getattr(L, "vcnf_vae_%s%s" % (k, sfx))
    return {
        "encode": (lambda p, b, s, d: f("encode")(p, FAKE, FAKE, FAKE, b, s, d, None), False),
        "encode_bwd": (lambda p, b, s, d: f("encode_bwd")(p, FAKE, FAKE, FAKE, FAKE, b, s, d, None), True),
        "gauss_z": (lambda p, n, s, d: f("gauss_log_prob")(p, FAKE, FAKE, n, 1, s, d, None), False),
        "gauss_x": (lambda p, n, s, d: f("gauss_log_prob")(p, FAKE, FAKE, n, s, 1, d, None), False),
        "gauss_z_bwd": (lambda p, n, s, d: f("gauss_log_prob_bwd")(p, FAKE, FAKE, FAKE, FAKE, n, 1, s, d, None), True),
        "gauss_x_bwd": (lambda p, n, s, d: f("gauss_log_prob_bwd")(p, FAKE, FAKE, FAKE, FAKE, n, s, 1, d, None), True),
        "bernoulli": (lambda p, n, s, d: f("bernoulli_log_prob")(p, FAKE, FAKE, n, s, d, None), False),
        "bernoulli_bwd": (lambda p, n, s, d: f("bernoulli_log_prob_bwd")(p, FAKE, FAKE, FAKE, n, s, d, None), True),
    }


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    for name, (call, limited) in _calls(L, sfx).items():
        rows = lambda b, s: b if name.startswith("encode") else b * s          # encode takes the batch, the others N
        assert call(None, rows(4, 3), 3, 8) == 1, name                # NULL required pointer
        assert call(None, rows(4, 3), 3, 0) == 1, name                # ... is looked at before the sizes
        assert call(FAKE, rows(4, 3), 3, 0) == 2, name                # D = 0
        assert call(FAKE, rows(4, 3), 3, -8) == 2, name
        assert call(FAKE, -1, 1, 8) == 2, name                        # negative count
        assert call(FAKE, rows(4, 3), 0, 8) == 2, name                # divisor / samples = 0
        assert call(FAKE, rows(4, 3), -3, 8) == 2, name
        assert call(ODD, rows(4, 3), 0, 8) == 2, name                 # ... the sizes before the alignment
        assert call(ODD, rows(4, 3), 3, 8) == 3, name                 # misaligned buffer
        assert call(ODD, rows(1, OVER), OVER, 8) == 3, name           # ... the alignment before the limit
        assert call(FAKE, 0, 3, 8) == 0, name                         # empty batch: no launch
        assert call(FAKE, 0, OVER, 8) == 0, name
        if limited:
            assert call(FAKE, rows(1, OVER), OVER, 8) == 5, name      # more samples than one lane may walk
        if not name.startswith("encode"):
            assert call(FAKE, 13, 3, 8) == 2, name                    # N % div != 0
    f = lambda k: getattr(L, "vcnf_vae_%s%s" % (k, sfx))
    # both divisors > 1
    assert f("gauss_log_prob")(FAKE, FAKE, FAKE, 12, 2, 3, 8, None) == 2
    assert f("gauss_log_prob_bwd")(FAKE, FAKE, FAKE, FAKE, FAKE, 12, 2, 3, 8, None) == 2
    # every required pointer, and the optional ones
    assert f("encode")(FAKE, None, FAKE, FAKE, 4, 3, 8, None) == 1
    assert f("encode")(FAKE, FAKE, None, FAKE, 4, 3, 8, None) == 1
    assert f("encode")(FAKE, FAKE, FAKE, None, 4, 3, 8, None) == 1
    assert f("encode")(FAKE, FAKE, FAKE, ODD, 4, 3, 8, None) == 3
    assert f("encode_bwd")(FAKE, FAKE, None, None, FAKE, 4, 3, 8, None) == 1           # both cotangents absent
    assert f("encode_bwd")(FAKE, FAKE, FAKE, FAKE, None, 4, 3, 8, None) == 1
    assert f("encode_bwd")(FAKE, FAKE, None, FAKE, FAKE, 0, 3, 8, None) == 0           # one cotangent is enough
    assert f("encode_bwd")(FAKE, FAKE, FAKE, None, FAKE, 0, 3, 8, None) == 0
    assert f("encode_bwd")(FAKE, FAKE, ODD, None, FAKE, 4, 3, 8, None) == 3
    assert f("gauss_log_prob")(FAKE, None, FAKE, 12, 1, 3, 8, None) == 1
    assert f("gauss_log_prob")(FAKE, FAKE, None, 12, 1, 3, 8, None) == 1
    assert f("gauss_log_prob_bwd")(FAKE, FAKE, None, FAKE, FAKE, 12, 1, 3, 8, None) == 1
    assert f("gauss_log_prob_bwd")(FAKE, FAKE, FAKE, None, None, 12, 1, 3, 8, None) == 1   # neither gradient wanted
    assert f("gauss_log_prob_bwd")(FAKE, FAKE, FAKE, None, FAKE, 0, 1, 3, 8, None) == 0
    assert f("gauss_log_prob_bwd")(FAKE, FAKE, FAKE, FAKE, None, 0, 3, 1, 8, None) == 0
    assert f("gauss_log_prob_bwd")(FAKE, FAKE, FAKE, FAKE, ODD, 12, 3, 1, 8, None) == 3
    assert f("bernoulli_log_prob")(FAKE, None, FAKE, 12, 3, 8, None) == 1
    assert f("bernoulli_log_prob")(FAKE, FAKE, None, 12, 3, 8, None) == 1
    assert f("bernoulli_log_prob_bwd")(FAKE, FAKE, None, FAKE, 12, 3, 8, None) == 1
    assert f("bernoulli_log_prob_bwd")(FAKE, FAKE, FAKE, None, 12, 3, 8, None) == 1
    # a shape that would need more than 2^31 - 1 workgroups
    assert f("bernoulli_log_prob")(FAKE, FAKE, FAKE, 1 << 40, 1, 1 << 20, None) == 2
    assert f("encode_bwd")(FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 40, 1, 1 << 20, None) == 2


def test_cpu_tensors_raise_in_the_wrappers():
    h, eps, v, g = torch.zeros(2, 8), torch.zeros(2, 3, 4), torch.zeros(6, 4), torch.zeros(6)
    for fn, args in ((_lib.vae_encode, (h, eps)), (_lib.vae_encode_bwd, (h, eps, eps, None)),
                     (_lib.vae_gauss_log_prob, (v, h, 1, 3)), (_lib.vae_gauss_log_prob_bwd, (v, h, g, 1, 3)),
                     (_lib.vae_bernoulli_log_prob, (v[:2], v, 3)), (_lib.vae_bernoulli_log_prob_bwd, (v[:2], v, g, 3))):
        with pytest.raises(nf.VcnfError):
            fn(*args)


# ---------------------------------------------------------------- the restatement against independent implementations
@pytest.mark.parametrize("shape", [7, (2, 3, 3)])
def test_restatement_matches_torch_normal(shape):
    b, s = 5, 3
    t = ref.inputs("encode", b, s, shape)
    mean, lv = ref.split(t["h"])
    normal = torch.distributions.Normal(mean.unsqueeze(1), torch.exp(0.5 * lv).unsqueeze(1))
    z, log_q = ref.encode(t["h"], t["eps"])
    assert z.shape == t["eps"].shape and log_q.shape == (b, s)
    assert_close(log_q, normal.log_prob(z).reshape(b, s, -1).sum(-1), what="encoder log_q", **PIN)
    # both roles of the Gaussian log-prob
    t = ref.inputs("gauss_z", b, s, shape)
    mean, lv = ref.split(ref.repeat_rows(t["h"], s))
    want = torch.distributions.Normal(mean, torch.exp(0.5 * lv)).log_prob(t["v"]).reshape(b * s, -1).sum(-1)
    assert_close(ref.gauss_log_prob(t["v"], t["h"], 1, s), want, what="log_prob(z, x)", **PIN)
    t = ref.inputs("gauss_x", b, s, shape)
    mean, lv = ref.split(t["h"])
    want = torch.distributions.Normal(mean, torch.exp(0.5 * lv)).log_prob(ref.repeat_rows(t["v"], s)).reshape(b * s, -1).sum(-1)
    assert_close(ref.gauss_log_prob(t["v"], t["h"], s, 1), want, what="decoder log_prob", **PIN)


def test_restatement_matches_binary_cross_entropy_with_logits():
    b, s = 5, 3
    t = ref.inputs("bernoulli", b, s, 7)
    assert float(t["x"][0].abs().max()) == 0.0 and float(t["x"][1].min()) == 1.0
    score = t["score"].clone()
    score[0, :4] = torch.tensor([80.0, -80.0, 1e4, -1e4], dtype=torch.float64)
    score[3, :4] = torch.tensor([80.0, -80.0, 1e4, -1e4], dtype=torch.float64)
    score[7, :4] = torch.tensor([80.0, -80.0, 1e4, -1e4], dtype=torch.float64)
    got = ref.bernoulli_log_prob(t["x"], score, s)
    want = -F.binary_cross_entropy_with_logits(score, ref.repeat_rows(t["x"], s), reduction="none").sum(-1)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    assert_close(got, want, what="bernoulli log_prob", **PIN)


# ---------------------------------------------------------------- modules
def test_public_names():
    D = nf.distributions
    assert nf.NormalizingFlowVAE is nf.core.NormalizingFlowVAE
    for name in ("BaseEncoder", "Dirac", "Uniform", "ConstDiagGaussian", "NNDiagGaussian"):
        assert getattr(D, name) is getattr(D.encoder, name)
    for name in ("BaseDecoder", "NNDiagGaussianDecoder", "NNBernoulliDecoder"):
        assert getattr(D, name) is getattr(D.decoder, name)
    assert all(issubclass(c, D.BaseEncoder) for c in (D.Dirac, D.Uniform, D.ConstDiagGaussian, D.NNDiagGaussian))
    assert all(issubclass(c, D.BaseDecoder) for c in (D.NNDiagGaussianDecoder, D.NNBernoulliDecoder))
    assert issubclass(D.BaseEncoder, nn.Module) and issubclass(D.BaseDecoder, nn.Module)
    assert not issubclass(nf.NormalizingFlowVAE, nf.NormalizingFlow)
    from vcnf_amd.autograd import VaeEncodeFn, VaeGaussLogProbFn, VaeBernoulliLogProbFn          # noqa: F401
    assert all(callable(getattr(_lib, "vae_" + k)) for k in KERNELS)
    with pytest.raises(TypeError):
        D.NNDiagGaussian(nn.Identity(), False)                        # fuse is keyword only
    with pytest.raises(TypeError):
        D.NNBernoulliDecoder(nn.Identity(), False)


def _model(n_flows=2, dtype=torch.float64, seed=3, fuse=True, prior=None):
    torch.manual_seed(seed)
    D = nf.distributions
    flows = [nf.flows.Planar(4, act="leaky_relu") for _ in range(n_flows)]
    model = nf.NormalizingFlowVAE(D.DiagGaussian(4) if prior is None else prior, D.NNDiagGaussian(nn.Linear(6, 8), fuse=fuse), flows,
                                  D.NNBernoulliDecoder(nn.Linear(4, 6), fuse=fuse))
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(0.5 * torch.randn(p.shape))
    return model.to(dtype)


def test_parameter_and_state_dict_names():
    model = _model()
    want = ["prior.loc", "prior.log_scale", "decoder.net.weight", "decoder.net.bias"] + \
           ["flows.%d.%s" % (i, n) for i in range(2) for n in "uwb"] + ["q0.net.weight", "q0.net.bias"]
    assert list(model.state_dict()) == want and [n for n, _ in model.named_parameters()] == want
    assert model.fuse_planar_stacks is True
    q = nf.distributions.ConstDiagGaussian([0.0, 1.0, 2.0], [1.0, 2.0, 0.5])
    assert [(n, tuple(p.shape)) for n, p in q.named_parameters()] == [("loc", (1, 1, 3)), ("scale", (1, 1, 3))]
    bare = nf.NormalizingFlowVAE(nf.distributions.DiagGaussian(4, trainable=False))
    assert isinstance(bare.q0, nf.distributions.Dirac) and bare.decoder is None and len(bare.flows) == 0
    assert list(bare.state_dict()) == ["prior.loc", "prior.log_scale"]
    # NormalizingFlow keeps its names and its switches
    flow = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), [nf.flows.Planar(2)])
    assert list(flow.state_dict()) == ["q0.loc", "q0.log_scale", "flows.0.u", "flows.0.w", "flows.0.b"]
    assert all(getattr(flow, s) is True for s, _, _ in nf.core._STACKS)


@pytest.mark.parametrize("s", [1, 3])
def test_output_shapes(s):
    D = nf.distributions
    x = torch.rand(5, 6, dtype=torch.float64)
    img = torch.rand(5, 2, 3, 3, dtype=torch.float64)
    for q, data, shape in ((D.Dirac(), x, (6,)), (D.Uniform(-1.0, 3.0), x, (6,)), (D.Dirac(), img, (2, 3, 3)),
                           (D.ConstDiagGaussian(torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)), x, (4,)),
                           (D.NNDiagGaussian(nn.Linear(6, 8).double()), x, (4,)),
                           (D.NNDiagGaussian(nn.Conv2d(2, 4, 1).double()), img, (2, 3, 3))):
        z, log_q = q(data, num_samples=s)
        assert z.shape == (5, s) + shape and log_q.shape == (5, s) and z.dtype == log_q.dtype == torch.float64, type(q)
        again = q.log_prob(z, data)
        assert again.shape == (5, s) and again.dtype == torch.float64
        if not isinstance(q, (D.Dirac, D.Uniform)):
            assert_close(again, log_q, what="log_prob of the draw", **PIN)
    u = D.Uniform(-1.0, 3.0)(x, s)
    assert float(u[0].min()) >= -1.0 and float(u[0].max()) < 3.0
    assert_close(u[1], torch.full((5, s), -1.3862943611198906, dtype=torch.float64), what="uniform log_q", **PIN)
    z = torch.randn(5 * s, 4, dtype=torch.float64)
    for dec, data in ((D.NNBernoulliDecoder(nn.Linear(4, 6).double()), x), (D.NNDiagGaussianDecoder(nn.Linear(4, 12).double()), x)):
        assert dec.log_prob(data, z).shape == (5 * s,)
    with torch.no_grad():
        mean, std = D.NNDiagGaussianDecoder(nn.Linear(4, 12).double())(z)
        probs = D.NNBernoulliDecoder(nn.Linear(4, 6).double())(z)
    assert mean.shape == std.shape == (5 * s, 6) and float(std.min()) > 0
    assert probs.shape == (5 * s, 6) and 0 <= float(probs.min()) and float(probs.max()) <= 1


def test_gaussian_decoder_counts_the_data_elements():
    """Deliberate deviation: the 2 pi constant uses the size of a data item and x is shared by its S rows."""
    D = nf.distributions
    dec = D.NNDiagGaussianDecoder(nn.Linear(4, 12).double())
    t = ref.inputs("gauss_x", 5, 3, 6)
    z = torch.randn(15, 4, dtype=torch.float64)
    with torch.no_grad():
        assert_close(dec.log_prob(t["v"], z), ref.gauss_log_prob(t["v"], dec.net(z), 3, 1), what="decoder", **PIN)


def test_cpu_model_is_the_restatement():
    b, s = 5, 3
    model = _model()
    x = torch.rand(b, 6, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    x[0], x[1] = 0.0, 1.0
    torch.manual_seed(11)
    z, log_q, log_p = model(x, num_samples=s)
    assert z.shape == (b, s, 4) and log_q.shape == (b, s) and log_p.shape == (b, s)
    (log_q.mean() - log_p.mean()).backward()
    torch.manual_seed(11)
    eps = torch.randn(b, s, 4, dtype=torch.float64)
    want, grads = ref.container_grads(model.state_dict(), x, eps, 2)
    for got, w, what in zip((z, log_q, log_p), want, ("z", "log_q", "log_p")):
        assert torch.isfinite(w).all()
        assert_close(got, w, what=what, **PIN)
    for name, p in model.named_parameters():
        assert p.grad is not None and float(p.grad.abs().sum()) > 0, name
        assert_close(p.grad, grads[name], what="d/d" + name, **PIN)
    # fuse=False is the same composition
    plain = _model(fuse=False)
    torch.manual_seed(11)
    for got, w in zip(plain(x, num_samples=s), want):
        assert_close(got, w, what="fuse=False", **PIN)
