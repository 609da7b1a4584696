"""Full-covariance bases without a GPU: the vcnf_mvn_* symbols are exported and bound, their host-side argument
validation returns the documented status codes before anything is launched, vcnf_mvn_bwd_groups is pure and keeps the
workspace bounded, the modules carry the stated parameter names, shapes and initial values, CPU tensors are refused, and
the plain-torch restatement the GPU tests compare against (mvn_ref.py) is itself pinned in fp64 to independent
implementations, on well-conditioned inputs."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import mvn_ref as ref
import vcnf_amd as nf
from helpers import assert_close
from vcnf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("log_prob", "sample", "log_prob_bwd", "sample_bwd", "reduce_partials")
FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
PIN = dict(rtol=1e-10, atol=1e-10)
CLASSES = {"gaussian": "MultivariateGaussian", "student_t": "MultivariateStudentT"}
# every (D, B) the GPU tests draw inputs for (test_gpu_mvn.py: CASES, the distribution test, the flow test)
SEEDED = [(1, 1000), (2, 1000), (7, 1000), (33, 1000), (64, 1000), (128, 1000), (7, 1), (7, 63), (128, 1), (8, 256)]


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    names = ["vcnf_mvn_%s%s" % (k, sfx) for k in KERNELS for sfx in ("_f32", "_f64")] + ["vcnf_mvn_bwd_groups"]
    for name in names:
        assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
        assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
    assert (_lib.MVN_GAUSSIAN, _lib.MVN_STUDENT_T) == (0, 1) and _lib.MVN_MAX_DIM == 128
    assert nf.lib().vcnf_abi_version() == 1


def _calls(L, sfx):
    """Per entry point a function (first pointer, batch, D, family) -> status, every other pointer valid."""
    lp = getattr(L, "vcnf_mvn_log_prob" + sfx)
    sa = getattr(L, "vcnf_mvn_sample" + sfx)
    lb = getattr(L, "vcnf_mvn_log_prob_bwd" + sfx)
    sb = getattr(L, "vcnf_mvn_sample_bwd" + sfx)
    return {
        "log_prob": lambda x, b, d, f: lp(x, FAKE, FAKE, FAKE, FAKE, b, d, f, 0, 1.0, None),
        "sample": lambda x, b, d, f: sa(x, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, b, d, f, None),
        "log_prob_bwd": lambda x, b, d, f: lb(x, FAKE, FAKE, FAKE, FAKE, None, FAKE, FAKE, b, d, f, None),
        "sample_bwd": lambda x, b, d, f: sb(x, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, b, d, f, None),
    }


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    for name, call in _calls(L, sfx).items():
        for family in (0, 1):
            assert call(None, 4, 8, family) == 1, name                 # NULL required pointer
            assert call(FAKE, 4, 0, family) == 2, name                 # features = 0
            assert call(FAKE, 4, 129, family) == 2, name               # beyond the limit
            assert call(FAKE, 0, 129, family) == 2, name
            assert call(FAKE, -1, 8, family) == 2, name
            assert call(ODD, 4, 8, family) == 3, name                  # misaligned buffer
            assert call(FAKE, 0, 8, family) == 0, name                 # empty batch: no launch
            assert call(FAKE, 0, 128, family) == 0, name
        assert call(FAKE, 4, 8, 2) == 5 and call(FAKE, 4, 8, -1) == 5, name      # unknown family
    lp = getattr(L, "vcnf_mvn_log_prob" + sfx)
    assert lp(FAKE, FAKE, FAKE, FAKE, None, 4, 8, 0, 0, 1.0, None) == 1                  # no logp
    assert lp(FAKE, FAKE, FAKE, None, FAKE, 4, 8, 0, 0, 1.0, None) == 1                  # no consts
    assert lp(FAKE, FAKE, None, FAKE, FAKE, 4, 8, 1, 0, 1.0, None) == 1                  # no tri_inv
    assert lp(FAKE, None, FAKE, FAKE, FAKE, 4, 8, 1, 0, 1.0, None) == 1                  # no loc
    assert lp(FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 0, 7, 1.0, None) == 5                  # unknown ld_mode
    assert lp(FAKE, FAKE, FAKE, FAKE, ODD, 4, 8, 0, 1, 1.0, None) == 3
    assert lp(FAKE, FAKE, ODD, FAKE, FAKE, 4, 8, 0, 1, 1.0, None) == 3
    sa = getattr(L, "vcnf_mvn_sample" + sfx)
    assert sa(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 1, None) == 1              # the t needs gamma
    assert sa(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, 0, 8, 0, None) == 0              # the Gaussian does not
    assert sa(FAKE, None, FAKE, FAKE, FAKE, None, FAKE, 4, 8, 0, None) == 1              # no z
    assert sa(FAKE, None, FAKE, FAKE, FAKE, FAKE, None, 4, 8, 0, None) == 1              # no logp
    assert sa(FAKE, ODD, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 1, None) == 3               # misaligned gamma
    lb = getattr(L, "vcnf_mvn_log_prob_bwd" + sfx)
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, None, None, FAKE, 4, 8, 0, None) == 1        # no dz
    assert lb(FAKE, FAKE, FAKE, FAKE, None, None, FAKE, FAKE, 4, 8, 0, None) == 1        # no cotangent
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, None, 0, 8, 0, None) == 0        # dz only: the workspace is optional
    assert lb(FAKE, FAKE, FAKE, FAKE, FAKE, ODD, FAKE, FAKE, 4, 8, 0, None) == 3         # misaligned gz_in
    sb = getattr(L, "vcnf_mvn_sample_bwd" + sfx)
    assert sb(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, FAKE, 4, 8, 1, None) == 1  # the t needs dgamma
    assert sb(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 1, None) == 1  # and gamma
    assert sb(FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 4, 8, 0, None) == 1  # no tri
    assert sb(FAKE, None, FAKE, FAKE, None, None, None, None, None, 0, 8, 0, None) == 0  # the Gaussian: all of them optional
    assert sb(FAKE, FAKE, FAKE, FAKE, ODD, FAKE, FAKE, FAKE, FAKE, 4, 8, 1, None) == 3   # misaligned g_z
    rp = getattr(L, "vcnf_mvn_reduce_partials" + sfx)
    assert rp(None, 4, 8, FAKE, FAKE, FAKE, None) == 1
    assert rp(FAKE, 4, 8, FAKE, FAKE, None, None) == 1
    assert rp(FAKE, 0, 8, FAKE, FAKE, FAKE, None) == 2                 # no blocks
    assert rp(FAKE, 4, 0, FAKE, FAKE, FAKE, None) == 2
    assert rp(FAKE, 4, 129, FAKE, FAKE, FAKE, None) == 2
    assert rp(ODD, 4, 8, FAKE, FAKE, FAKE, None) == 3


def test_bwd_groups_is_a_pure_function_of_the_shape():
    """One workgroup per 64 samples, at most 256, and at most 2^22 elements of partial blocks (include/vcnf_hip.h)."""
    L = nf.lib()
    for b, d in [(1, 1), (63, 7), (64, 7), (65, 7), (1000, 1), (1000, 128), (8192, 128), (1 << 20, 2), (1 << 20, 64), (1 << 20, 128)]:
        n = L.vcnf_mvn_bwd_groups(b, d)
        assert n == L.vcnf_mvn_bwd_groups(b, d) == min((b + 63) // 64, 256, (1 << 22) // (d * d + d + 1)), (b, d)
        assert 1 <= n <= 256 and n * (d * d + d + 1) <= 1 << 22
    assert L.vcnf_mvn_bwd_groups(1000, 128) >= 2
    for b, d in [(4096, 0), (-1, 8), (4096, 129)]:
        assert L.vcnf_mvn_bwd_groups(b, d) == 0


def test_lds_layout_header_compiles_on_its_own(tmp_path):
    """csrc/mvn_lds.hpp is plain C++17: its static_asserts (every launch fits a CU, every block of the outer-product sum
    has an owner, the quoted byte counts) hold, and the layout's regions are ordered for every D."""
    exe = str(tmp_path / "mvn_lds_check")
    cmd = ["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "vcnf_amd", "csrc"),
           os.path.join(ROOT, "tests", "c_host", "mvn_lds_check.cpp"), "-o", exe]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    assert "mvn_lds_check ok (128 sizes x 2 types x 2 layouts)" in run.stdout


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_state_dict_names_shapes_and_initial_values(family):
    cls = getattr(nf.distributions, CLASSES[family])
    names = ["loc", "log_diag", "lower"] + (["log_df"] if family == "student_t" else [])
    q = cls(5)
    assert list(q.state_dict()) == names
    shapes = {"loc": (1, 5), "log_diag": (1, 5), "lower": (5, 5), "log_df": (1,)}
    assert all(tuple(v.shape) == shapes[k] for k, v in q.state_dict().items())
    assert [n for n, _ in q.named_parameters()] == names and not list(q.buffers())
    assert q.n_dim == 5 and isinstance(q, nf.distributions.BaseDistribution) and not hasattr(q, "temperature")
    assert all(p.dtype == torch.get_default_dtype() for p in q.parameters())
    for k in ("loc", "log_diag", "lower"):
        assert float(getattr(q, k).detach().abs().max()) == 0.0, k
    assert torch.equal(q.scale_tril.detach(), torch.eye(5))
    if family == "student_t":
        assert torch.allclose(q.log_df.detach(), torch.tensor([math.log(3.0)]), rtol=0, atol=1e-7)
        assert torch.allclose(cls(2, df=1.5).log_df.detach(), torch.tensor([math.log(1.5)]), rtol=0, atol=1e-7)
    # a given location and scale factor
    tril = np.array([[1.5, 0.0, 0.0], [0.3, 0.5, 0.0], [-0.2, 0.1, 2.0]])
    q = cls(3, loc=[1.0, -2.0, 0.5], scale_tril=tril).double()
    assert q.lower.dtype == torch.float64
    assert_close(q.scale_tril, tril, rtol=0, atol=1e-7, what="scale_tril")
    assert_close(q.loc, [[1.0, -2.0, 0.5]], rtol=0, atol=1e-7, what="loc")
    assert float(q.lower.detach().triu().abs().max()) == 0.0
    with pytest.raises(AttributeError):
        q.scale_tril = torch.eye(3)
    model = nf.NormalizingFlow(cls(2), [nf.flows.Permute(2, "swap")])
    assert list(model.state_dict())[:len(names)] == ["q0." + n for n in names]


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_untrainable_base_has_buffers_only(family):
    names = ["loc", "log_diag", "lower"] + (["log_df"] if family == "student_t" else [])
    q = getattr(nf.distributions, CLASSES[family])(3, trainable=False)
    assert not list(q.parameters())
    assert list(q.state_dict()) == names
    assert [n for n, _ in q.named_buffers()] == names


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_bad_arguments_raise(family):
    cls = getattr(nf.distributions, CLASSES[family])
    for bad in ([[1.0, 0.5], [0.0, 1.0]],            # an upper entry
                [[1.0, 0.0], [0.5, 0.0]],            # a zero on the diagonal
                [[1.0, 0.0], [0.5, -1.0]],           # a negative one
                np.eye(3)):                          # the wrong size
        with pytest.raises(ValueError):
            cls(2, scale_tril=bad)
    with pytest.raises(ValueError):
        cls(2, loc=[0.0, 1.0, 2.0])
    if family == "student_t":
        for df in (0.0, -1.0):
            with pytest.raises(ValueError):
                cls(2, df=df)
    q = cls(129)
    for call in (lambda: q.log_prob(torch.zeros(2, 129)), lambda: q.from_noise(torch.zeros(2, 129)), lambda: q(2)):
        with pytest.raises(NotImplementedError, match="128"):
            call()


def test_public_names():
    from vcnf_amd.distributions import MultivariateGaussian, MultivariateStudentT          # noqa: F401
    from vcnf_amd.autograd import MultivariateLogProbFn, MultivariateSampleFn             # noqa: F401
    assert all(callable(f) for f in (_lib.mvn_log_prob, _lib.mvn_sample, _lib.mvn_log_prob_bwd, _lib.mvn_sample_bwd))
    for mod in (nf, nf.distributions):
        assert not hasattr(mod, "TMV") and not hasattr(mod, "MVN")            # no alias under the fork's names


@pytest.mark.parametrize("trainable", [True, False])
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_cpu_tensors_raise(family, trainable):
    q = getattr(nf.distributions, CLASSES[family])(4, trainable=trainable)
    x = torch.zeros(5, 4)
    with pytest.raises(nf.VcnfError):
        q.log_prob(x)
    with pytest.raises(nf.VcnfError):
        q.from_noise(x)
    if family == "student_t":
        with pytest.raises(nf.VcnfError):
            q.from_noise(x, torch.ones(5))
    with pytest.raises(nf.VcnfError):
        q(5)
    row, tri, consts, fam = torch.zeros(4), torch.eye(4), torch.tensor([0.0, 3.0]), _lib.MVN_STUDENT_T
    for fn, args in ((_lib.mvn_log_prob, (x, row, tri, consts, fam)),
                     (_lib.mvn_sample, (x, x[:, 0] + 1, row, tri, consts, fam)),
                     (_lib.mvn_log_prob_bwd, (x, row, tri, consts, fam, x[:, 0])),
                     (_lib.mvn_sample_bwd, (x, x[:, 0] + 1, tri, consts, fam, x, x[:, 0]))):
        with pytest.raises(nf.VcnfError):
            fn(*args)


# ---------------------------------------------------------------- the restatement against independent implementations
@pytest.mark.parametrize("d", [1, 7, 33])
def test_restatement_matches_torch_multivariate_normal(d):
    p, eps, _, z = ref.inputs("gaussian", d)
    mvn = torch.distributions.MultivariateNormal(p["loc"][0], scale_tril=ref.scale_tril(p))
    got = ref.log_prob("gaussian", z, p)
    print("restatement vs torch.distributions.MultivariateNormal: max difference %.3e" % float((got - mvn.log_prob(z)).abs().max()))
    assert_close(got, mvn.log_prob(z), what="log_prob", **PIN)
    # the sampling form: the density of its z is the density it returns
    zs, lp = ref.sample("gaussian", eps, None, p)
    assert_close(lp, mvn.log_prob(zs), what="sample log_p", **PIN)


@pytest.mark.parametrize("d", [2, 7, 33])
def test_restatement_matches_scipy_multivariate_t(d):
    stats = pytest.importorskip("scipy.stats")
    p, eps, gamma, z = ref.inputs("student_t", d)
    L = ref.scale_tril(p).numpy()
    dist = stats.multivariate_t(loc=p["loc"][0].numpy(), shape=L @ L.T, df=float(torch.exp(p["log_df"])))
    got = ref.log_prob("student_t", z, p)
    print("restatement vs scipy.stats.multivariate_t: max difference %.3e" % float((got - torch.as_tensor(dist.logpdf(z.numpy()))).abs().max()))
    assert_close(got, dist.logpdf(z.numpy()), what="log_prob", **PIN)
    zs, lp = ref.sample("student_t", eps, gamma, p)
    assert_close(lp, dist.logpdf(zs.numpy()), what="sample log_p", **PIN)


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_restatement_at_lower_zero_is_the_diagonal_formula(family):
    p, _, _, z = ref.inputs(family, 7)
    p = dict(p, lower=torch.zeros_like(p["lower"]))
    u = (z - p["loc"]) / torch.exp(p["log_diag"])
    q = (u * u).sum(1)
    if family == "gaussian":
        want = (-0.5 * math.log(2 * math.pi) - p["log_diag"] - 0.5 * u * u).sum(1)
    else:
        nu = torch.exp(p["log_df"][0])
        want = (torch.lgamma(0.5 * (nu + 7)) - torch.lgamma(0.5 * nu) - 3.5 * torch.log(nu * math.pi) - p["log_diag"].sum()
                - 0.5 * (nu + 7) * torch.log1p(q / nu))
    assert_close(ref.log_prob(family, z, p), want, what="lower = 0", **PIN)


def test_restatement_t_in_one_dimension_matches_torch_student_t():
    p, eps, gamma, z = ref.inputs("student_t", 1)
    dist = torch.distributions.StudentT(torch.exp(p["log_df"]), p["loc"][0], torch.exp(p["log_diag"][0]))
    assert_close(ref.log_prob("student_t", z, p), dist.log_prob(z)[:, 0], what="log_prob", **PIN)
    zs, lp = ref.sample("student_t", eps, gamma, p)
    assert_close(lp, dist.log_prob(zs)[:, 0], what="sample log_p", **PIN)


def test_seeded_inputs_are_well_conditioned():
    """cond(L) <= 20 for every seeded input the tests use, so that the inverse the build multiplies with and the solve of
    the restatement agree to the working precision."""
    for family in ref.FAMILIES:
        for d, b in SEEDED:
            p, eps, gamma, z = ref.inputs(family, d, b)
            cond = float(torch.linalg.cond(ref.scale_tril(p)))
            print("%s D = %d: cond(L) = %.2f" % (family, d, cond))
            assert cond <= 20.0, (family, d, cond)
            assert z.shape == (b, d) and torch.isfinite(z).all() and float(p["lower"].triu().abs().max()) == 0.0
            assert (gamma is None) == (family == "gaussian")
