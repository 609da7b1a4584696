"""MultivariateGaussian and MultivariateStudentT base distributions on the HIP kernels (csrc/mvn_base.hip).

The reference is the plain-torch restatement in mvn_ref.py (a triangular solve, never the inverse), run on the CPU in fp32
and in fp64 on the inputs as the module sees them.  fp32 results are judged by helpers.parity (against the restatement's
fp32 run, with its own fp32-vs-fp64 error as the yardstick); fp64 results by rtol = atol = 1e-10.  Inputs are seeded
(mvn_ref.inputs): loc ~ 2 N(0, 1), log_diag ~ 0.3 N(0, 1), strictly lower entries ~ 0.5 N(0, 1) / sqrt(D), nu log-uniform
on [1.5, 30], z the distribution's own draw with the first B / 8 rows multiplied by 5.  Before anything is compared the
restatement's outputs are checked to be finite in both precisions."""
import functools
import math

import pytest
import torch

import mvn_ref as ref
import vcnf_amd as nf
from helpers import assert_close, parity
from vcnf_amd import _lib

pytestmark = pytest.mark.gpu

# no off-diagonal entry (1), a width that takes no pack (7), just past a 32-lane boundary (33), the launch above 64 KiB
# of LDS (128; fp64 from 64 on), a single sample, a partial wave, a partial last tile (1000 = 15 x 64 + 40)
CASES = [(1, 1000), (2, 1000), (7, 1000), (33, 1000), (64, 1000), (128, 1000), (7, 1), (7, 63), (128, 1)]
F64 = dict(rtol=1e-10, atol=1e-10)
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
CLASSES = {"gaussian": "MultivariateGaussian", "student_t": "MultivariateStudentT"}
FAMILY_ID = {"gaussian": _lib.MVN_GAUSSIAN, "student_t": _lib.MVN_STUDENT_T}
cast = ref.cast


def case_id(case):
    return "D%d-B%d" % case


def references(fn, dtype, *tensors):
    """fn on the CPU: (fp32 run or None, fp64 run) of the inputs rounded to ``dtype``; every output finite."""
    seen = [cast(t, dtype) for t in tensors]
    r64 = fn(*[cast(t, torch.float64) for t in seen])
    r32 = fn(*[cast(t, torch.float32) for t in seen]) if dtype == torch.float32 else None
    for r in (r64, r32):
        for t in ((r if isinstance(r, (tuple, list)) else (r,)) if r is not None else ()):
            assert torch.isfinite(t).all(), "the reference output is not finite"
    return r32, r64


def check(got, r32, r64, dtype, what):
    got = got.reshape(r64.shape)
    if dtype == torch.float32:
        assert got.dtype == torch.float32
        parity(got, r32, r64, what=what)
    else:
        assert got.dtype == torch.float64
        assert_close(got, r64, what=what, **F64)


def build(family, d, p, dtype, trainable=True):
    q = getattr(nf.distributions, CLASSES[family])(d, trainable=trainable).to(dtype)
    q.load_state_dict(cast(p, dtype))
    return q.cuda()


def cuda(t, dtype):
    return None if t is None else cast(t, dtype).cuda()


def operands(q):
    """(loc [D], L, L^-1, consts) as the module hands them to the kernels"""
    with torch.no_grad():
        tri = q.scale_tril
        return q.loc.reshape(-1), tri, q._inverse(tri), q._consts()


def nan_above(tri):
    return tri.masked_fill(torch.ones_like(tri, dtype=torch.bool).triu(1), float("nan"))


@functools.lru_cache(maxsize=None)
def log_prob_reference(family, d, b, dtype):
    p, _, _, z = ref.inputs(family, d, b)
    return references(lambda z_, p_: ref.log_prob(family, z_, p_), dtype, z, p)


@functools.lru_cache(maxsize=None)
def sample_reference(family, d, b, dtype):
    p, eps, gamma, _ = ref.inputs(family, d, b)
    return references(lambda e, g, p_: ref.sample(family, e, g, p_), dtype, eps, gamma, p)


# ---------------------------------------------------------------- 1. log_prob
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_log_prob(hip, family, case, dtype):
    d, b = case
    p, _, _, z = ref.inputs(family, d, b)
    r32, r64 = log_prob_reference(family, d, b, dtype)
    q = build(family, d, p, dtype)
    zc = cuda(z, dtype)
    loc, _, tri_inv, consts = operands(q)
    fam = FAMILY_ID[family]
    with torch.no_grad():
        lp = q.log_prob(zc)
        acc = torch.full((b,), 2.0, dtype=dtype, device="cuda")
        assert q.log_prob(zc, out=acc) is acc
        again = q.log_prob(zc)
        # ld_mode / sign through the wrapper: store -log_p, accumulate -log_p
        neg = _lib.mvn_log_prob(zc, loc, tri_inv, consts, fam, sign=-1.0)
        sub = _lib.mvn_log_prob(zc, loc, tri_inv, consts, fam, logp=torch.full((b,), 2.0, dtype=dtype, device="cuda"), sign=-1.0)
        # only the lower triangle of the operand is read
        holes = _lib.mvn_log_prob(zc, loc, nan_above(tri_inv), consts, fam)
    assert lp.shape == (b,) and lp.dtype == dtype
    print("%s %s %s max |log_p - fp64 reference| %.3e of %.3e" % (family, case, dtype, float((lp.cpu().double() - r64).abs().max()),
                                                                 float(r64.abs().max())))
    check(lp, r32, r64, dtype, "log_prob")
    # accumulation into an existing buffer: one more rounding of 2 +- log_p
    one = 2e-7 if dtype == torch.float32 else 1e-15
    assert_close(acc, 2.0 + lp.double().cpu(), rtol=one, atol=0, what="log_prob(out=)")
    assert_close(sub, 2.0 - lp.double().cpu(), rtol=one, atol=0, what="accumulate, sign = -1")
    assert torch.equal(neg, -lp), "sign = -1 is not the negated log_p"
    assert torch.equal(again, lp), "the same call twice gives different bits"
    assert torch.equal(holes, lp), "NaN above the diagonal of the operand changes the result"


# ---------------------------------------------------------------- 2. from_noise
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_from_noise(hip, family, case, dtype):
    d, b = case
    p, eps, gamma, _ = ref.inputs(family, d, b)
    r32, r64 = sample_reference(family, d, b, dtype)
    q = build(family, d, p, dtype)
    args = (cuda(eps, dtype),) + ((cuda(gamma, dtype),) if gamma is not None else ())
    loc, tri, _, consts = operands(q)
    with torch.no_grad():
        z, lp = q.from_noise(*args)
        z2, lp2 = q.from_noise(*args)
        back = q.log_prob(z)
        zh, lh = _lib.mvn_sample(args[0], args[1] if gamma is not None else None, loc, nan_above(tri), consts, FAMILY_ID[family])
        zf, lf = q(33)
        zn, ln = q.from_noise(args[0])
    assert z.shape == eps.shape and lp.shape == (b,) and z.dtype == dtype and lp.dtype == dtype
    check(z, r32 and r32[0], r64[0], dtype, "from_noise z")
    check(lp, r32 and r32[1], r64[1], dtype, "from_noise log_p")
    assert torch.equal(z2, z) and torch.equal(lp2, lp)
    assert torch.equal(zh, z) and torch.equal(lh, lp), "NaN above the diagonal of the operand changes the result"
    print("%s %s %s max |log_prob(z) - log_p| %.3e" % (family, case, dtype, float((back - lp).abs().max())))
    check(back, r32 and r32[1], r64[1], dtype, "log_prob(z) of the returned z")
    for zz, ll, n in ((zf, lf, 33), (zn, ln, b)):
        assert zz.shape == (n, d) and ll.shape == (n,) and zz.dtype == dtype
        assert torch.isfinite(zz).all() and torch.isfinite(ll).all()


# ---------------------------------------------------------------- 3. gradients
def _weights(b):
    return torch.linspace(0.5, 1.5, b, dtype=torch.float64)


def _z_cotangent(b, d):
    """unit-scale, fixed"""
    return torch.cos(0.37 * torch.arange(b * d, dtype=torch.float64)).reshape(b, d)


def _loss(direction, log_prob, sample, x, gamma, w, gz, scale):
    if direction == "log_prob":
        return (log_prob(x) * w).sum() * scale
    z, lp = sample(x, gamma)
    return ((lp * w).sum() + (z * gz).sum()) * scale


def _ref_grads(family, direction, dtype, p, x, gamma, scale):
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    p = {k: leaf(v) for k, v in p.items()}
    x = leaf(x)
    gamma = leaf(gamma) if gamma is not None and direction == "sample" else None
    b, d = x.shape
    loss = _loss(direction, lambda z_: ref.log_prob(family, z_, p), lambda e, g: ref.sample(family, e, g, p), x, gamma,
                 _weights(b).to(dtype), _z_cotangent(b, d).to(dtype), scale)
    loss.backward()
    out = {"input": x.grad}
    if gamma is not None:
        out["log_gamma"] = gamma.grad * gamma.detach()
    out.update({k: v.grad for k, v in p.items()})
    return out


def _hip_grads(q, direction, x, gamma, scale):
    q.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    gamma = gamma.clone().requires_grad_() if gamma is not None and direction == "sample" else None
    b, d = x.shape
    sample = (lambda e, g: q.from_noise(e, g)) if gamma is not None else (lambda e, g: q.from_noise(e))
    loss = _loss(direction, q.log_prob, sample, x, gamma, _weights(b).to(x), _z_cotangent(b, d).to(x), scale)
    loss.backward()
    out = {"input": x.grad}
    if gamma is not None:
        # compared as the gradient with respect to log gamma: gamma reaches far below 1, the raw one has no scale
        out["log_gamma"] = gamma.grad * gamma.detach()
    out.update({k: v.grad for k, v in q.named_parameters()})
    return {k: (None if v is None else v.clone()) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def gradient_reference(family, d, b, direction, dtype, scaled):
    """(fp32 or None, fp64) autograd gradients of the restatement on the CPU; computed once per case."""
    p, eps, gamma, z = ref.inputs(family, d, b)
    x = eps if direction == "sample" else z
    p, x, gamma = cast(p, dtype), x.to(dtype), cast(gamma, dtype)
    scale = 1.0 / b if scaled else 1.0
    r64 = _ref_grads(family, direction, torch.float64, p, x, gamma, scale)
    r32 = _ref_grads(family, direction, torch.float32, p, x, gamma, scale) if dtype == torch.float32 else None
    for r in (r64, r32):
        assert r is None or all(torch.isfinite(v).all() for v in r.values()), "the reference gradient is not finite"
    return r32, r64


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("scaled", [False, True], ids=["unit", "mean"])
@pytest.mark.parametrize("direction", ["log_prob", "sample"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_gradients_match_autograd_on_the_restatement(hip, family, case, direction, scaled, dtype):
    """Loss sum_b w_b log_p_b, w = linspace(0.5, 1.5, B), plus sum z . v (v of unit scale) through from_noise, as it is
    and divided by B: gradients with respect to z (eps and log gamma when sampling), loc, log_diag, lower and log_df.
    The gradient of lower is exactly zero on and above the diagonal.  Two backward passes: equal bits."""
    d, b = case
    p, eps, gamma, z = ref.inputs(family, d, b)
    r32, r64 = gradient_reference(family, d, b, direction, dtype, scaled)
    q = build(family, d, p, dtype)
    groups = _lib.lib().vcnf_mvn_bwd_groups(b, d)
    assert groups >= (2 if b == 1000 else 1)
    args = (direction, cuda(eps if direction == "sample" else z, dtype), cuda(gamma, dtype), 1.0 / b if scaled else 1.0)
    got, again = _hip_grads(q, *args), _hip_grads(q, *args)
    assert sorted(got) == sorted(r64)
    for k in got:
        assert torch.equal(got[k], again[k]), "gradient of %s differs between two backward passes" % k
    for k in sorted(r64):
        assert got[k] is not None and got[k].dtype == dtype and got[k].shape == r64[k].shape, k
        print("%s %s %s %s d/d%s max |got - fp64 reference| %.3e of %.3e" % (
            family, case, direction, dtype, k, float((got[k].cpu().double() - r64[k]).abs().max()), float(r64[k].abs().max())))
    assert float(got["lower"].triu().abs().max()) == 0.0, "the gradient of lower is not zero on and above the diagonal"
    for k in sorted(r64):
        check(got[k], r32 and r32[k], r64[k], dtype, "d/d" + k)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(7, 63), (33, 1000), (128, 1000)], ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_log_prob_vjp_adds_the_incoming_gradient(hip, family, case, dtype):
    """vcnf_mvn_log_prob_bwd_* with gz_in: dz = gz_in + g dlogp/dz, the parameter sums unchanged; without the sums the
    same dz."""
    d, b = case
    p, eps, _, z = ref.inputs(family, d, b)
    r32, r64 = gradient_reference(family, d, b, "log_prob", dtype, False)
    q = build(family, d, p, dtype)
    zc, w, gz = cuda(z, dtype), cuda(_weights(b), dtype), cuda(eps, dtype)
    loc, _, tri_inv, consts = operands(q)
    fam = FAMILY_ID[family]
    with torch.no_grad():
        plain = _lib.mvn_log_prob_bwd(zc, loc, tri_inv, consts, fam, w)
        added = _lib.mvn_log_prob_bwd(zc, loc, nan_above(tri_inv), consts, fam, w, gz_in=gz)
        only = _lib.mvn_log_prob_bwd(zc, loc, tri_inv, consts, fam, w, gz_in=gz, sums=False)
    want64 = r64["input"] + cast(eps, dtype).double()
    want32 = r32["input"] + eps.float() if dtype == torch.float32 else None
    check(added[0], want32, want64, dtype, "dz with gz_in")
    check(plain[0], r32 and r32["input"], r64["input"], dtype, "dz")
    check(plain[1], r32 and r32["loc"][0], r64["loc"][0], dtype, "d_loc")
    assert torch.equal(only[0], added[0]) and only[1:] == (None, None, None)
    for a, c in zip(plain[1:], added[1:]):
        assert torch.equal(a, c)
    assert float(plain[2].triu(1).abs().max()) == 0.0 and torch.isfinite(plain[2]).all()


# ---------------------------------------------------------------- 4. the drawn distribution
def _kolmogorov_p(samples, cdf):
    """Asymptotic p-value of the two-sided Kolmogorov-Smirnov statistic (Stephens' small-sample correction)."""
    x, _ = torch.sort(samples.double())
    n = len(x)
    f = cdf(x)
    i = torch.arange(1, n + 1, dtype=torch.float64)
    stat = float(torch.maximum(i / n - f, f - (i - 1) / n).max())
    lam = (math.sqrt(n) + 0.12 + 0.11 / math.sqrt(n)) * stat
    p = 2.0 * sum((-1.0) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam) for k in range(1, 101))
    return stat, min(max(p, 0.0), 1.0)


def _chi2_cdf(d):
    return lambda q: torch.special.gammainc(torch.full_like(q, 0.5 * d), 0.5 * q)


def _f_cdf(d, nu, points=400001):
    """CDF of F(d, nu) at x: I_u(d/2, nu/2) with u = d x / (d x + nu).  With v = (1 - u)^b the incomplete beta integral
    is (1 / b) int_{(1-u)^b}^1 (1 - v^(1/b))^(a-1) dv, a bounded integrand: cumulative trapezoid on a uniform grid."""
    a, b = 0.5 * d, 0.5 * nu
    v = torch.linspace(0.0, 1.0, points, dtype=torch.float64)
    y = (1.0 - v ** (1.0 / b)).clamp_min(0.0) ** (a - 1.0)
    area = torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(0.5 * (y[1:] + y[:-1]) * (v[1] - v[0]), 0)])
    log_beta = math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)

    def cdf(x):
        u = d * x / (d * x + nu)
        at = ((1.0 - u) ** b) * (points - 1)
        lo = at.floor().clamp(0, points - 2).long()
        upto = area[lo] + (at - lo) * (area[lo + 1] - area[lo])
        return ((area[-1] - upto) / b / math.exp(log_beta)).clamp(0.0, 1.0)
    return cdf


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_forward_draws_the_stated_distribution(hip, family, seed=11):
    """20 000 draws at D = 7, mapped back through the fp64 restatement to q = |L^-1 (z - loc)|^2: q ~ chi^2_D for the
    Gaussian and q / D ~ F(D, nu) for the t, Kolmogorov-Smirnov p > 1e-4.  A gamma concentration of nu for nu / 2, or a
    draw per element for one per sample, is off by far more."""
    n, d = 20000, 7
    p = ref.inputs(family, d)[0]
    q = build(family, d, p, torch.float32)
    torch.manual_seed(seed)
    with torch.no_grad():
        z, lp = q(n)
    assert z.shape == (n, d) and lp.shape == (n,) and torch.isfinite(z).all() and torch.isfinite(lp).all()
    p32 = cast(cast(p, torch.float32), torch.float64)
    maha = ref.mahalanobis(z.cpu().double(), p32)
    if family == "gaussian":
        stat, pv = _kolmogorov_p(maha, _chi2_cdf(d))
    else:
        stat, pv = _kolmogorov_p(maha / d, _f_cdf(d, float(torch.exp(p32["log_df"]))))
    print("%s seed %d: Kolmogorov-Smirnov statistic %.5f, p = %.4f" % (family, seed, stat, pv))
    assert pv > 1e-4
    # the returned density is that of the returned draw
    assert_close(lp, ref.log_prob(family, z.cpu().double(), p32), rtol=1e-4, atol=1e-3, what="log_p of the draw")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_log_df_gradient_includes_the_path_through_gamma(hip, dtype):
    """forward(n) draws gamma with autograd on.  With the same draws supplied as constants the gradient of log_df lacks
    sum_b dgamma_b dgamma/dconcentration dconcentration/dlog_df, torch's implicit derivative of its gamma sampler; the
    two differ by exactly that term.  Sums of n = 256 terms in the module's dtype: 1e-4 / 1e-10 of the gradient."""
    n, d = 256, 8
    p = ref.inputs("student_t", d, 256)[0]
    q = build("student_t", d, p, dtype)
    loss = lambda z, lp: lp.sum() + 0.1 * (z * z).sum()

    torch.manual_seed(5)
    z, lp = q(n)
    loss(z, lp).backward()
    full = q.log_df.grad.clone()
    q.zero_grad(set_to_none=True)

    torch.manual_seed(5)
    eps = torch.randn(n, d, dtype=dtype, device="cuda")
    conc = (0.5 * torch.exp(q.log_df.detach())).expand(n)
    gamma = torch._standard_gamma(conc).requires_grad_()
    z2, lp2 = q.from_noise(eps, gamma)
    assert torch.equal(z2, z) and torch.equal(lp2, lp)
    loss(z2, lp2).backward()
    cut = q.log_df.grad.clone()
    path = (gamma.grad * torch._standard_gamma_grad(conc, gamma.detach())).sum(0, keepdim=True) * conc[:1]      # d(nu / 2)/dlog nu = nu / 2
    assert torch.isfinite(full).all() and float(path.abs().max()) > 0
    scale = float(full.abs().max())
    assert_close(full, (cut + path).cpu(), rtol=0, atol=(1e-4 if dtype == torch.float32 else 1e-10) * scale, what="d/dlog_df")
    assert float((full - cut).abs().max()) > 1e-3 * scale, "the gamma path contributes nothing"


# ---------------------------------------------------------------- 5. in a flow
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_flow_log_prob_objectives_and_a_step(hip, family, dtype):
    """NormalizingFlow(base, [CoupledRationalQuadraticSpline(8, 1, 32), Permute(8, 'swap')]), B = 256, against the same
    model with the base replaced by the restatement: log_prob(x) is the layers walked by hand plus the restated base
    term; forward_kld is its mean, and its gradients with respect to the base's parameters are autograd's on the
    restatement at the same z; reverse_kld (against a fixed DiagGaussian) reaches every parameter with a finite
    gradient.  One Adam step changes lower only below the diagonal."""
    n, d = 256, 8
    torch.manual_seed(41)
    p = cast(cast(ref.inputs(family, d, 256)[0], torch.float32), dtype)
    q0 = getattr(nf.distributions, CLASSES[family])(d)
    q0.load_state_dict(cast(p, torch.float32))
    model = nf.NormalizingFlow(q0, [nf.flows.CoupledRationalQuadraticSpline(8, 1, 32), nf.flows.Permute(8, "swap")]).to(dtype).cuda()
    model.eval()
    g = torch.Generator().manual_seed(43)
    x = (1.5 * torch.randn(n, d, generator=g, dtype=torch.float64)).to(dtype)
    with torch.no_grad():
        lp = model.log_prob(x.cuda())
        z, log_det = x.cuda(), torch.zeros(n, dtype=dtype, device="cuda")
        for flow in reversed(model.flows):
            z, ld = flow.inverse(z)
            log_det = log_det + ld
    z, log_det = z.cpu(), log_det.cpu()
    want = {dt: log_det.to(dt) + ref.log_prob(family, z.to(dt), cast(p, dt)) for dt in (torch.float32, torch.float64)}
    assert all(torch.isfinite(v).all() for v in want.values())
    check(lp, want[torch.float32], want[torch.float64], dtype, "NormalizingFlow.log_prob")

    model.train()
    loss = model.forward_kld(x.cuda())
    loss.backward()
    assert_close(loss, -want[torch.float64].mean(), rtol=1e-5 if dtype == torch.float32 else 1e-10,
                 atol=1e-5 if dtype == torch.float32 else 1e-10, what="forward_kld")
    grads = {}
    for dt in (torch.float32, torch.float64):
        leaves = {k: v.to(dt).clone().requires_grad_() for k, v in p.items()}
        (-ref.log_prob(family, z.to(dt), leaves).mean()).backward()
        grads[dt] = {k: v.grad for k, v in leaves.items()}
    for name, par in model.q0.named_parameters():
        assert par.grad is not None and torch.isfinite(par.grad).all() and float(par.grad.abs().sum()) > 0, name
        check(par.grad, grads[torch.float32][name], grads[torch.float64][name], dtype, "forward_kld d/d" + name)
    assert float(model.q0.lower.grad.triu().abs().max()) == 0.0

    model.zero_grad(set_to_none=True)
    model.p = nf.distributions.DiagGaussian(d, trainable=False).to(dtype).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    before = model.q0.lower.detach().clone()
    torch.manual_seed(3)
    loss = model.reverse_kld(256)
    loss.backward()
    assert torch.isfinite(loss)
    for name, par in model.named_parameters():
        assert par.grad is not None and torch.isfinite(par.grad).all(), name
    for name, par in model.q0.named_parameters():
        assert float(par.grad.abs().sum()) > 0, name
    opt.step()
    moved = model.q0.lower.detach() != before
    assert bool(moved.tril(-1).any()) and not bool(moved.triu().any()), "the step changed lower on or above the diagonal"
    assert torch.isfinite(model.q0.scale_tril).all()
