"""Class-conditional bases without a GPU: the vcnf_cc_gaussian_* symbols are exported and bound, their host-side
argument validation returns the documented status codes before anything is launched, the modules carry the
reference's parameter names and shapes, and CPU tensors are refused."""
import ctypes

import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib

KERNELS = ("log_prob", "sample", "log_prob_bwd", "sample_bwd", "reduce_rows")
FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    for k in KERNELS:
        for sfx in ("_f32", "_f64"):
            name = "vcnf_cc_gaussian_%s%s" % (k, sfx)
            assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
            assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]


def _calls(L, sfx):
    """Per entry point a function (first pointer, batch, C, P, R, row_index) -> status, every other pointer valid."""
    lp = getattr(L, "vcnf_cc_gaussian_log_prob" + sfx)
    sa = getattr(L, "vcnf_cc_gaussian_sample" + sfx)
    lb = getattr(L, "vcnf_cc_gaussian_log_prob_bwd" + sfx)
    sb = getattr(L, "vcnf_cc_gaussian_sample_bwd" + sfx)
    return {
        "log_prob": lambda x, b, c, p, r, idx: lp(x, FAKE, FAKE, idx, 0.0, FAKE, b, c, p, r, 0, 1.0, None),
        "sample": lambda x, b, c, p, r, idx: sa(x, FAKE, FAKE, idx, 0.0, FAKE, FAKE, b, c, p, r, None),
        "log_prob_bwd": lambda x, b, c, p, r, idx: lb(x, FAKE, FAKE, idx, 0.0, FAKE, FAKE, FAKE, FAKE, b, c, p, r, None),
        "sample_bwd": lambda x, b, c, p, r, idx: sb(x, FAKE, idx, 0.0, FAKE, FAKE, FAKE, FAKE, FAKE, b, c, p, r, None),
    }


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    for name, call in _calls(L, sfx).items():
        assert call(None, 4, 8, 4, 1, None) == 1, name                 # NULL required pointer
        assert call(FAKE, 4, 0, 4, 1, None) == 2, name                 # channels < 1
        assert call(FAKE, 4, 8, 0, 1, None) == 2, name                 # pixels < 1
        assert call(FAKE, 4, 8, 4, 3, None) == 2, name                 # 3 table rows for a batch of 4, no row_index
        assert call(FAKE, 4, 8, 4, 0, FAKE) == 2, name                 # empty table
        assert call(ODD, 4, 8, 4, 1, None) == 3, name                  # misaligned buffer
        assert call(FAKE, 4, 8, 4, 4, ODD) == 3, name                  # misaligned row_index
        assert call(FAKE, 0, 8, 4, 1, None) == 0, name                 # empty batch: no launch
        assert call(FAKE, 0, 8, 4, 10, FAKE) == 0, name
    lp = getattr(L, "vcnf_cc_gaussian_log_prob" + sfx)
    assert lp(FAKE, FAKE, FAKE, None, 0.0, None, 4, 8, 4, 1, 0, 1.0, None) == 1       # no logp
    assert lp(FAKE, FAKE, FAKE, None, 0.0, FAKE, 4, 8, 4, 1, 7, 1.0, None) == 5       # unknown ld_mode
    sa = getattr(L, "vcnf_cc_gaussian_sample" + sfx)
    assert sa(FAKE, FAKE, FAKE, None, 0.0, None, FAKE, 4, 8, 4, 1, None) == 1         # sample without z
    rr = getattr(L, "vcnf_cc_gaussian_reduce_rows" + sfx)
    assert rr(FAKE, None, FAKE, 4, 8, 10, None) == 1
    assert rr(FAKE, FAKE, FAKE, 4, 0, 10, None) == 2
    assert rr(FAKE, FAKE, FAKE, 4, 8, 0, None) == 2
    assert rr(ODD, FAKE, FAKE, 4, 8, 10, None) == 3


def _shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def test_class_cond_diag_gaussian_parameters():
    q = nf.distributions.ClassCondDiagGaussian((6, 4, 4), 10)
    assert _shapes(q) == {"loc": (6, 4, 4, 10), "log_scale": (6, 4, 4, 10)}
    assert all(float(p.detach().abs().sum()) == 0.0 for p in q.parameters())
    assert q.temperature is None and q.d == 96 and q.shape == (6, 4, 4)
    assert _shapes(nf.distributions.ClassCondDiagGaussian(8, 3)) == {"loc": (8, 3), "log_scale": (8, 3)}


def test_glow_base_parameters():
    per_channel = {k: (1, 12, 1, 1) for k in ("loc", "loc_logs", "log_scale", "log_scale_logs")}
    q = nf.distributions.GlowBase((12, 8, 8), 10)
    assert _shapes(q) == dict(per_channel, loc_cc=(10, 12), log_scale_cc=(10, 12))
    assert list(q.state_dict()) == ["loc", "loc_logs", "log_scale", "log_scale_logs", "loc_cc", "log_scale_cc"]
    assert all(float(p.detach().abs().sum()) == 0.0 for p in q.parameters())
    assert q.temperature is None and q.num_pix == 64 and q.d == 768 and q.class_cond and q.logscale_factor == 3.
    plain = nf.distributions.GlowBase((12, 8, 8))
    assert _shapes(plain) == per_channel and not plain.class_cond
    assert _shapes(nf.distributions.GlowBase(7, 4)) == {"loc": (1, 7), "loc_logs": (1, 7), "log_scale": (1, 7),
                                                       "log_scale_logs": (1, 7), "loc_cc": (4, 7), "log_scale_cc": (4, 7)}


def test_public_names():
    from vcnf_amd import ClassCondFlow                                                    # noqa: F401
    from vcnf_amd.distributions import ClassCondDiagGaussian, GlowBase                    # noqa: F401
    from vcnf_amd.autograd import ClassCondGaussianLogProbFn, ClassCondGaussianSampleFn   # noqa: F401
    assert issubclass(ClassCondDiagGaussian, nf.distributions.BaseDistribution)
    model = nf.ClassCondFlow(ClassCondDiagGaussian(8, 10), [nf.flows.Permute(8, "swap")])
    assert "q0.loc" in model.state_dict()


@pytest.mark.parametrize("make", [lambda: nf.distributions.ClassCondDiagGaussian(8, 10),
                                  lambda: nf.distributions.GlowBase((4, 2, 2), 10),
                                  lambda: nf.distributions.GlowBase((4, 2, 2))])
def test_cpu_tensors_raise(make):
    q = make()
    x = torch.zeros((3,) + q.shape)
    y = torch.tensor([0, 1, 2])
    with pytest.raises(nf.VcnfError):
        q.log_prob(x, y)
    with pytest.raises(nf.VcnfError):
        q.from_noise(x, y)
    with pytest.raises(nf.VcnfError):
        q(3, y)


def test_class_cond_flow_cpu_raises():
    model = nf.ClassCondFlow(nf.distributions.ClassCondDiagGaussian(8, 10), [])
    with pytest.raises(nf.VcnfError):
        model.log_prob(torch.zeros(3, 8), torch.tensor([0, 1, 2]))


def test_multiscale_keeps_class_cond_and_refuses_unsupported_bases():
    q0 = [nf.distributions.GlowBase((4, 2, 2), 10)]
    assert nf.MultiscaleFlow(q0, [[]], [], class_cond=True).class_cond
    assert not nf.MultiscaleFlow(q0, [[]], [], class_cond=False).class_cond
    with pytest.raises(NotImplementedError):
        nf.MultiscaleFlow([nf.distributions.BaseDistribution()], [[]], [])
