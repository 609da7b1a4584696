"""Heavy-tailed bases without a GPU: the vcnf_tail_* symbols are exported and bound, their host-side argument validation
returns the documented status codes before anything is launched, the modules carry the stated parameter names, shapes
and initial values, CPU tensors are refused, and the plain-torch restatement the GPU tests compare against
(heavy_tail_ref.py) is itself pinned in fp64 to independent implementations."""
import ctypes
import math

import numpy as np
import pytest
import torch

import heavy_tail_ref as ref
import vcnf_amd as nf
from helpers import assert_close
from vcnf_amd import _lib

KERNELS = ("log_prob", "sample", "log_prob_bwd", "sample_bwd", "reduce_partials")
FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
PIN = dict(rtol=1e-10, atol=1e-10)
CLASSES = {"student_t": ("StudentT", "log_df", "df", 3.0), "gen_gaussian": ("GeneralizedGaussian", "log_beta", "beta", 2.0)}


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    names = ["vcnf_tail_%s%s" % (k, sfx) for k in KERNELS for sfx in ("_f32", "_f64")] + ["vcnf_tail_bwd_groups"]
    for name in names:
        assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
        assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    assert (_lib.TAIL_STUDENT_T, _lib.TAIL_GEN_GAUSSIAN) == (0, 1)


def _calls(L, sfx):
    """Per entry point a function (first pointer, batch, D, family) -> status, every other pointer valid."""
    lp = getattr(L, "vcnf_tail_log_prob" + sfx)
    sa = getattr(L, "vcnf_tail_sample" + sfx)
    lb = getattr(L, "vcnf_tail_log_prob_bwd" + sfx)
    sb = getattr(L, "vcnf_tail_sample_bwd" + sfx)
    return {
        "log_prob": lambda x, b, d, f: lp(x, FAKE, FAKE, FAKE, FAKE, FAKE, b, d, f, 0, 1.0, None),
        "sample": lambda x, b, d, f: sa(x, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, b, d, f, None),
        "log_prob_bwd": lambda x, b, d, f: lb(x, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, b, d, f, None),
        "sample_bwd": lambda x, b, d, f: sb(x, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, b, d, f, None),
    }


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    for name, call in _calls(L, sfx).items():
        for family in (0, 1):
            assert call(None, 4, 8, family) == 1, name                 # NULL required pointer
            assert call(FAKE, 4, 0, family) == 2, name                 # features = 0
            assert call(FAKE, -1, 8, family) == 2, name
            assert call(ODD, 4, 8, family) == 3, name                  # misaligned buffer
            assert call(FAKE, 0, 8, family) == 0, name                 # empty batch: no launch
            assert call(FAKE, 0, 1 << 20, family) == 0, name           # no upper limit on the features
        assert call(FAKE, 4, 8, 2) == 5 and call(FAKE, 4, 8, -1) == 5, name      # unknown family
    lp = getattr(L, "vcnf_tail_log_prob" + sfx)
    assert lp(FAKE, FAKE, FAKE, FAKE, FAKE, None, 4, 8, 0, 0, 1.0, None) == 1            # no logp
    assert lp(FAKE, FAKE, FAKE, FAKE, None, FAKE, 4, 8, 0, 0, 1.0, None) == 1            # no cst
    assert lp(FAKE, FAKE, FAKE, None, FAKE, FAKE, 4, 8, 1, 0, 1.0, None) == 1            # no shape row
    assert lp(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 0, 7, 1.0, None) == 5            # unknown ld_mode
    assert lp(FAKE, FAKE, FAKE, FAKE, FAKE, ODD, 4, 8, 0, 1, 1.0, None) == 3
    sa = getattr(L, "vcnf_tail_sample" + sfx)
    assert sa(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 0, None) == 1        # sample without gamma
    assert sa(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 4, 8, 1, None) == 1        # sample without z
    assert sa(FAKE, ODD, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 1, None) == 3         # misaligned gamma
    lb = getattr(L, "vcnf_tail_log_prob_bwd" + sfx)
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, None, None, FAKE, 4, 8, 0, None) == 1        # no dz
    assert lb(FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE, 4, 8, 0, None) == 1        # no cotangent
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, None, 0, 8, 0, None) == 0        # dz only: the workspace is optional
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, ODD, FAKE, FAKE, 4, 8, 0, None) == 3         # misaligned gz_in
    sb = getattr(L, "vcnf_tail_sample_bwd" + sfx)
    assert sb(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 4, 8, 0, None) == 1      # no dgamma
    assert sb(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 0, None) == 1      # no gamma
    assert sb(FAKE, FAKE, FAKE, FAKE, FAKE, None, None, None, FAKE, None, 0, 8, 1, None) == 0      # cotangents, deps, workspace optional
    assert sb(FAKE, FAKE, FAKE, FAKE, FAKE, ODD, FAKE, FAKE, FAKE, FAKE, 4, 8, 1, None) == 3       # misaligned g_z
    rp = getattr(L, "vcnf_tail_reduce_partials" + sfx)
    assert rp(None, 4, 8, FAKE, FAKE, FAKE, None) == 1
    assert rp(FAKE, 4, 8, FAKE, FAKE, None, None) == 1
    assert rp(FAKE, 0, 8, FAKE, FAKE, FAKE, None) == 2                 # no blocks
    assert rp(FAKE, 4, 0, FAKE, FAKE, FAKE, None) == 2
    assert rp(ODD, 4, 8, FAKE, FAKE, FAKE, None) == 3


def test_bwd_groups_is_a_pure_function_of_the_shape():
    L = nf.lib()
    for b, d in [(1, 1), (63, 7), (4096, 64), (4096, 257), (4096, 4099), (1 << 20, 2), (1 << 20, 64), (1 << 20, 1 << 20)]:
        n = L.vcnf_tail_bwd_groups(b, d)
        assert n >= 1 and n == L.vcnf_tail_bwd_groups(b, d), (b, d)
        assert n * 3 * d <= max(1 << 21, 128 * 3 * d)                  # the workspace stays bounded
    assert L.vcnf_tail_bwd_groups(4096, 0) == 0 and L.vcnf_tail_bwd_groups(-1, 8) == 0


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_state_dict_names_shapes_and_initial_values(family):
    cls, tail, kw, default = CLASSES[family]
    q = getattr(nf.distributions, cls)((3, 4, 4))
    assert list(q.state_dict()) == ["loc", "log_scale", tail]
    assert all(tuple(v.shape) == (1, 3, 4, 4) for v in q.state_dict().values())
    assert [n for n, _ in q.named_parameters()] == ["loc", "log_scale", tail] and not list(q.buffers())
    assert q.shape == (3, 4, 4) and q.d == 48 and isinstance(q, nf.distributions.BaseDistribution)
    assert all(p.dtype == torch.get_default_dtype() for p in q.parameters())
    assert float(q.loc.detach().abs().max()) == 0.0 and float(q.log_scale.detach().abs().max()) == 0.0
    assert torch.allclose(getattr(q, tail).detach(), torch.full((1, 3, 4, 4), math.log(default)), rtol=0, atol=1e-7)
    # an int shape, a float and an array for the tail parameter
    q = getattr(nf.distributions, cls)(5, **{kw: 1.5})
    assert q.shape == (5,) and torch.allclose(getattr(q, tail).detach(), torch.full((1, 5), math.log(1.5)), rtol=0, atol=1e-7)
    values = np.linspace(0.7, 2.4, 6).reshape(2, 3)
    q = getattr(nf.distributions, cls)((2, 3), **{kw: values}).double()
    assert getattr(q, tail).dtype == torch.float64
    assert_close(getattr(q, tail)[0], np.log(values), rtol=0, atol=1e-7, what=tail)
    with pytest.raises(ValueError):
        getattr(nf.distributions, cls)(3, **{kw: [1.0, 0.0, 2.0]})
    model = nf.NormalizingFlow(getattr(nf.distributions, cls)(2), [nf.flows.Permute(2, "swap")])
    assert list(model.state_dict())[:3] == ["q0.loc", "q0.log_scale", "q0." + tail]


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_untrainable_base_has_buffers_only(family):
    cls, tail, _, _ = CLASSES[family]
    q = getattr(nf.distributions, cls)(3, trainable=False)
    assert not list(q.parameters())
    assert list(q.state_dict()) == ["loc", "log_scale", tail]
    assert [n for n, _ in q.named_buffers()] == ["loc", "log_scale", tail]


def test_public_names():
    from vcnf_amd.distributions import StudentT, GeneralizedGaussian                   # noqa: F401
    from vcnf_amd.autograd import HeavyTailLogProbFn, HeavyTailSampleFn                # noqa: F401
    assert all(callable(f) for f in (_lib.tail_log_prob, _lib.tail_sample, _lib.tail_log_prob_bwd, _lib.tail_sample_bwd))
    assert not hasattr(nf.distributions, "T") and not hasattr(nf.distributions, "GGD")     # no alias under the fork's names


@pytest.mark.parametrize("trainable", [True, False])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_cpu_tensors_raise(family, trainable):
    q = getattr(nf.distributions, CLASSES[family][0])(4, trainable=trainable)
    x = torch.zeros(5, 4)
    with pytest.raises(nf.VcnfError):
        q.log_prob(x)
    with pytest.raises(nf.VcnfError):
        q.from_noise(x)
    with pytest.raises(nf.VcnfError):
        q.from_noise(x, torch.ones(5, 4))
    with pytest.raises(nf.VcnfError):
        q(5)
    row = torch.zeros(4)
    fam = _lib.TAIL_STUDENT_T
    for fn, args in ((_lib.tail_log_prob, (x, row, row, row + 1, row, fam)),
                     (_lib.tail_sample, (x, x + 1, row, row, row + 1, row, fam)),
                     (_lib.tail_log_prob_bwd, (x, row, row, row + 1, fam, x[:, 0])),
                     (_lib.tail_sample_bwd, (x, x + 1, row, row, row + 1, fam, x, x[:, 0]))):
        with pytest.raises(nf.VcnfError):
            fn(*args)


# ---------------------------------------------------------------- the restatement against independent implementations
def test_restatement_matches_torch_student_t():
    p, eps, gamma, z = ref.inputs("student_t", 7)
    want = torch.distributions.StudentT(torch.exp(p["log_df"]), p["loc"], torch.exp(p["log_scale"])).log_prob(z).sum(1)
    got = ref.log_prob("student_t", z, p)
    print("restatement vs torch.distributions.StudentT: max difference %.3e" % float((got - want).abs().max()))
    assert_close(got, want, what="log_prob", **PIN)
    # the sampling form: the density of its z is the density it returns
    zs, lp = ref.sample("student_t", eps, gamma, p)
    assert_close(lp, torch.distributions.StudentT(torch.exp(p["log_df"]), p["loc"], torch.exp(p["log_scale"])).log_prob(zs).sum(1),
                 what="sample log_p", **PIN)


def test_restatement_matches_scipy_gennorm():
    stats = pytest.importorskip("scipy.stats")
    p, eps, gamma, z = ref.inputs("gen_gaussian", 7)
    want = stats.gennorm.logpdf(z.numpy(), torch.exp(p["log_beta"]).numpy(), loc=p["loc"].numpy(),
                                scale=torch.exp(p["log_scale"]).numpy()).sum(1)
    got = ref.log_prob("gen_gaussian", z, p)
    print("restatement vs scipy.stats.gennorm: max difference %.3e" % float((got - torch.as_tensor(want)).abs().max()))
    assert_close(got, want, what="log_prob", **PIN)


def test_restatement_at_beta_two_is_a_gaussian():
    p, eps, gamma, z = ref.inputs("gen_gaussian", 7)
    p = dict(p, log_beta=torch.full_like(p["log_beta"], math.log(2.0)))
    sigma = torch.exp(p["log_scale"]) / math.sqrt(2.0)
    want = (-0.5 * math.log(2 * math.pi) - torch.log(sigma) - 0.5 * ((z - p["loc"]) / sigma) ** 2).sum(1)
    assert_close(ref.log_prob("gen_gaussian", z, p), want, what="beta = 2", **PIN)
    # the sampling form at beta = 2: gamma ~ Gamma(1/2, 1) is u^2, and the returned density is that of the returned z
    zs, lp = ref.sample("gen_gaussian", eps, gamma, p)
    assert_close(lp, (-0.5 * math.log(2 * math.pi) - torch.log(sigma) - 0.5 * ((zs - p["loc"]) / sigma) ** 2).sum(1),
                 what="sample log_p at beta = 2", **PIN)


def test_restatement_normaliser_is_fp64_whatever_the_dtype():
    """c(nu) in fp32 arithmetic loses digits as nu grows (two lgamma values of size nu log nu cancel to O(log nu)); the
    restatement's fp32 run carries the fp64 value rounded once."""
    log_df = torch.tensor([math.log(3.0), math.log(30.0), math.log(3000.0)])
    c64 = ref.normaliser("student_t", log_df.double())
    c32 = ref.normaliser("student_t", log_df)
    assert c32.dtype == torch.float32
    assert float((c32.double() - c64).abs().max()) <= 1.2e-7 * float(c64.abs().max())
