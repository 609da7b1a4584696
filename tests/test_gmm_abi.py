"""Gaussian mixture base without a GPU: the vcnf_gmm_* symbols are exported and bound, their host-side argument
validation returns the documented status codes before anything is launched, the module carries the reference's
parameter names, shapes and initial values, and CPU tensors are refused."""
import ctypes
import math

import numpy as np
import pytest
import torch

import vcnf_amd as nf
from vcnf_amd import _lib

KERNELS = ("log_prob", "sample", "log_prob_bwd", "reduce_partials")
FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    names = ["vcnf_gmm_%s%s" % (k, sfx) for k in KERNELS for sfx in ("_f32", "_f64")] + ["vcnf_gmm_bwd_groups"]
    for name in names:
        assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
        assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]


def _calls(L, sfx):
    """Per entry point a function (first pointer, batch, D, M) -> status, every other pointer valid."""
    lp = getattr(L, "vcnf_gmm_log_prob" + sfx)
    sa = getattr(L, "vcnf_gmm_sample" + sfx)
    lb = getattr(L, "vcnf_gmm_log_prob_bwd" + sfx)
    return {
        "log_prob": lambda x, b, d, m: lp(x, FAKE, FAKE, FAKE, FAKE, b, d, m, 0, 1.0, None),
        "sample": lambda x, b, d, m: sa(x, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, b, d, m, None),
        "log_prob_bwd": lambda x, b, d, m: lb(x, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, b, d, m, None),
    }


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    for name, call in _calls(L, sfx).items():
        assert call(None, 4, 8, 3) == 1, name                          # NULL required pointer
        assert call(FAKE, 4, 0, 3) == 2, name                          # D = 0
        assert call(FAKE, 4, 8, 0) == 2, name                          # M = 0
        assert call(FAKE, 4, 129, 64) == 2, name                       # M * D = 8256 > 8192
        assert call(FAKE, -1, 8, 3) == 2, name
        assert call(ODD, 4, 8, 3) == 3, name                           # misaligned buffer
        assert call(FAKE, 0, 8, 3) == 0, name                          # empty batch: no launch
        assert call(FAKE, 0, 64, 128) == 0, name                       # M * D = 8192 is inside the range
    lp = getattr(L, "vcnf_gmm_log_prob" + sfx)
    assert lp(FAKE, FAKE, FAKE, FAKE, None, 4, 8, 3, 0, 1.0, None) == 1            # no logp
    assert lp(FAKE, FAKE, FAKE, None, FAKE, 4, 8, 3, 0, 1.0, None) == 1            # no log_w
    assert lp(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 3, 7, 1.0, None) == 5            # unknown ld_mode
    assert lp(FAKE, FAKE, FAKE, FAKE, ODD, 4, 8, 3, 1, 1.0, None) == 3
    sa = getattr(L, "vcnf_gmm_sample" + sfx)
    assert sa(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 3, None) == 1        # sample without modes
    assert sa(FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 4, 8, 3, None) == 1        # sample without z
    assert sa(FAKE, ODD, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 3, None) == 3         # misaligned modes
    lb = getattr(L, "vcnf_gmm_log_prob_bwd" + sfx)
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, FAKE, 4, 8, 3, None) == 1      # no dz
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, None, 0, 8, 3, None) == 0      # dz only: the workspace is optional
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, ODD, FAKE, FAKE, 4, 8, 3, None) == 3       # misaligned gz_in
    rp = getattr(L, "vcnf_gmm_reduce_partials" + sfx)
    assert rp(None, 4, 3, 8, FAKE, FAKE, FAKE, None) == 1
    assert rp(FAKE, 4, 3, 8, FAKE, FAKE, None, None) == 1
    assert rp(FAKE, 0, 3, 8, FAKE, FAKE, FAKE, None) == 2              # no blocks
    assert rp(FAKE, 4, 0, 8, FAKE, FAKE, FAKE, None) == 2
    assert rp(FAKE, 4, 3, 0, FAKE, FAKE, FAKE, None) == 2
    assert rp(FAKE, 4, 64, 129, FAKE, FAKE, FAKE, None) == 2
    assert rp(ODD, 4, 3, 8, FAKE, FAKE, FAKE, None) == 3


def test_bwd_groups_is_a_pure_function_of_the_shape():
    L = nf.lib()
    for b, d, m in [(1, 1, 1), (63, 7, 5), (4096, 64, 16), (1 << 20, 2, 8), (1 << 20, 30, 64), (1 << 20, 8192, 1)]:
        n = L.vcnf_gmm_bwd_groups(b, d, m)
        assert n >= 1 and n == L.vcnf_gmm_bwd_groups(b, d, m), (b, d, m)
        assert n * m * (2 * d + 1) <= max(1 << 23, 256 * m * (2 * d + 1))     # the workspace stays bounded
    assert L.vcnf_gmm_bwd_groups(4096, 129, 64) == 0                           # outside the supported range


def test_state_dict_names_shapes_and_initial_values():
    q = nf.distributions.GaussianMixture(5, 7)
    assert list(q.state_dict()) == ["loc", "log_scale", "weight_scores"]
    assert {k: tuple(v.shape) for k, v in q.state_dict().items()} == {
        "loc": (1, 5, 7), "log_scale": (1, 5, 7), "weight_scores": (1, 5)}
    assert [n for n, _ in q.named_parameters()] == ["loc", "log_scale", "weight_scores"] and not list(q.buffers())
    assert q.n_modes == 5 and q.dim == 7 and isinstance(q, nf.distributions.BaseDistribution)
    assert all(p.dtype == torch.get_default_dtype() for p in q.parameters())
    assert float(q.log_scale.detach().abs().max()) == 0.0
    assert torch.allclose(q.weight_scores.detach(), torch.full((1, 5), math.log(1.0 / 5)), rtol=0, atol=1e-7)
    assert float(q.loc.detach().std()) > 0.1                           # a standard-normal draw, not zeros


def test_untrainable_mixture_has_buffers_only():
    q = nf.distributions.GaussianMixture(3, 2, trainable=False)
    assert not list(q.parameters())
    assert list(q.state_dict()) == ["loc", "log_scale", "weight_scores"]
    assert [n for n, _ in q.named_buffers()] == ["loc", "log_scale", "weight_scores"]


def test_given_parameters_are_stored_as_stated():
    loc = [[0.5, -1.0], [2.0, 3.0]]
    scale = [[1.0, 2.0], [0.5, 4.0]]
    q = nf.distributions.GaussianMixture(2, 2, loc=loc, scale=scale, weights=[1, 3])
    assert torch.equal(q.loc.detach(), torch.tensor([loc]))
    assert torch.allclose(q.log_scale.detach(), torch.log(torch.tensor([scale])), rtol=0, atol=1e-7)
    assert torch.allclose(q.weight_scores.detach(), torch.log(torch.tensor([[0.25, 0.75]])), rtol=0, atol=1e-7)
    d = nf.distributions.GaussianMixture(2, 2, loc=np.array(loc), scale=np.array(scale), weights=np.array([1., 3.])).double()
    assert d.loc.dtype == torch.float64 and tuple(d.weight_scores.shape) == (1, 2)
    model = nf.NormalizingFlow(q, [nf.flows.Permute(2, "swap")])
    assert list(model.state_dict())[:3] == ["q0.loc", "q0.log_scale", "q0.weight_scores"]


def test_public_names():
    from vcnf_amd.distributions import GaussianMixture                                  # noqa: F401
    from vcnf_amd.autograd import GaussianMixtureLogProbFn, GaussianMixtureSampleFn    # noqa: F401
    assert callable(_lib.gmm_log_prob) and callable(_lib.gmm_sample) and callable(_lib.gmm_log_prob_bwd)


@pytest.mark.parametrize("trainable", [True, False])
def test_cpu_tensors_raise(trainable):
    q = nf.distributions.GaussianMixture(3, 4, trainable=trainable)
    x = torch.zeros(5, 4)
    with pytest.raises(nf.VcnfError):
        q.log_prob(x)
    with pytest.raises(nf.VcnfError):
        q.from_noise(x)
    with pytest.raises(nf.VcnfError):
        q.from_noise(x, torch.zeros(5, dtype=torch.long))
    with pytest.raises(nf.VcnfError):
        q(5)
    for fn, args in ((_lib.gmm_log_prob, (x, q.loc[0], q.log_scale[0], q.weight_scores[0])),
                     (_lib.gmm_sample, (x, torch.zeros(5, dtype=torch.int32), q.loc[0], q.log_scale[0], q.weight_scores[0])),
                     (_lib.gmm_log_prob_bwd, (x, q.loc[0], q.log_scale[0], q.weight_scores[0], x[:, 0], x[:, 0]))):
        with pytest.raises(nf.VcnfError):
            fn(*[a.detach() for a in args])


def test_tables_beyond_the_kernel_limit_are_refused_by_name():
    q = nf.distributions.GaussianMixture(64, 129, trainable=False)
    with pytest.raises(NotImplementedError, match="8192"):
        q._tables()
