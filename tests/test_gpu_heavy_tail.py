"""StudentT and GeneralizedGaussian base distributions on the HIP kernels (csrc/heavy_tail.hip).

The reference is the plain-torch restatement in heavy_tail_ref.py, run on the CPU in fp32 and in fp64 on the inputs as
the module sees them.  fp32 results are judged by helpers.parity (against the restatement's fp32 run, with its own
fp32-vs-fp64 error as the yardstick); fp64 results by rtol = atol = 1e-10.  Inputs are seeded (heavy_tail_ref.inputs):
loc ~ 2 N(0, 1), log_scale ~ 0.3 N(0, 1), nu log-uniform on [1.5, 30], beta uniform on [0.6, 2.5], z the distribution's
own draw (B = 4096) with the first B / 8 rows multiplied by 25.  Before anything is compared the restatement's outputs are
checked to be finite in both precisions."""
import functools
import math

import pytest
import torch

import heavy_tail_ref as ref
import vcnf_amd as nf
from helpers import assert_close, parity
from vcnf_amd import _lib

pytestmark = pytest.mark.gpu

B = 4096
# one lane group with a tail (1, 2, 7), non-vector-width rows (7, 257, 4099), rows longer than a lane group's registers
# (257 in scalar accesses, 4099), an image shape, and batches that leave the last workgroup partial
CASES = [(1, B), (2, B), (7, B), (64, B), (257, B), (4099, B), ((3, 4, 4), B), (7, 1), (7, 63)]
F64 = dict(rtol=1e-10, atol=1e-10)
QUANTILE_LIMIT = 1 << 24
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
CLASSES = {"student_t": "StudentT", "gen_gaussian": "GeneralizedGaussian"}
FAMILY_ID = {"student_t": _lib.TAIL_STUDENT_T, "gen_gaussian": _lib.TAIL_GEN_GAUSSIAN}
cast = ref.cast


def case_id(case):
    return "%s-B%d" % (str(case[0]).replace(" ", ""), case[1])


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
        # parity's percentile (torch.quantile) takes at most 2^24 elements: the largest case is judged in runs of rows,
        # each of which has to pass on its own
        step = max(1, QUANTILE_LIMIT // max(1, r64[0].numel())) if r64.dim() > 1 and r64.numel() > QUANTILE_LIMIT else len(r64)
        for i in range(0, len(r64), max(1, step)):
            parity(got[i:i + step], r32[i:i + step], r64[i:i + step], what=what)
    else:
        assert got.dtype == torch.float64
        assert_close(got, r64, what=what, **F64)


def build(family, shape, p, dtype, trainable=True):
    q = getattr(nf.distributions, CLASSES[family])(shape, trainable=trainable).to(dtype)
    q.load_state_dict(cast(p, dtype))
    return q.cuda()


def cuda(t, dtype):
    return cast(t, dtype).cuda()


def rows(q):
    with torch.no_grad():
        return [r.detach() for r in q._rows()[:4]]


def log_prob_reference(family, shape, b, dtype):
    p, _, _, z = ref.inputs(family, shape, b)
    return references(lambda z_, p_: ref.log_prob(family, z_, p_), dtype, z, p)


def sample_reference(family, shape, b, dtype):
    p, eps, gamma, _ = ref.inputs(family, shape, b)
    return references(lambda e, g, p_: ref.sample(family, e, g, p_), dtype, eps, gamma, p)


# ---------------------------------------------------------------- 1. log_prob
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_log_prob(hip, family, case, dtype):
    shape, b = case
    p, _, _, z = ref.inputs(family, shape, b)
    r32, r64 = log_prob_reference(family, shape, b, dtype)
    q = build(family, shape, p, dtype)
    zc = cuda(z, dtype)
    with torch.no_grad():
        lp = q.log_prob(zc)
        acc = torch.full((b,), 2.0, dtype=dtype, device="cuda")
        assert q.log_prob(zc, out=acc) is acc
        again = q.log_prob(zc)
        # ld_mode / sign through the wrapper: store -log_p, accumulate -log_p
        neg = _lib.tail_log_prob(zc, *rows(q), FAMILY_ID[family], sign=-1.0)
        sub = _lib.tail_log_prob(zc, *rows(q), FAMILY_ID[family], logp=torch.full((b,), 2.0, dtype=dtype, device="cuda"), sign=-1.0)
    assert lp.shape == (b,) and lp.dtype == dtype
    print("%s %s %s max |log_p - fp64 reference| %.3e" % (family, case, dtype, float((lp.cpu().double() - r64).abs().max())))
    check(lp, r32, r64, dtype, "log_prob")
    # accumulation into an existing buffer: one more rounding of 2 +- log_p
    one = 2e-7 if dtype == torch.float32 else 1e-15
    assert_close(acc, 2.0 + lp.double().cpu(), rtol=one, atol=0, what="log_prob(out=)")
    assert_close(sub, 2.0 - lp.double().cpu(), rtol=one, atol=0, what="accumulate, sign = -1")
    assert torch.equal(neg, -lp), "sign = -1 is not the negated log_p"
    assert torch.equal(again, lp), "the same call twice gives different bits"


# ---------------------------------------------------------------- 2. from_noise
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_from_noise(hip, family, case, dtype):
    shape, b = case
    p, eps, gamma, _ = ref.inputs(family, shape, b)
    r32, r64 = sample_reference(family, shape, b, dtype)
    q = build(family, shape, p, dtype)
    with torch.no_grad():
        z, lp = q.from_noise(cuda(eps, dtype), cuda(gamma, dtype))
        z2, lp2 = q.from_noise(cuda(eps, dtype), cuda(gamma, dtype))
        back = q.log_prob(z)
        zf, lf = q(33)
        zn, ln = q.from_noise(cuda(eps, dtype))
    assert z.shape == eps.shape and lp.shape == (b,) and z.dtype == dtype and lp.dtype == dtype
    check(z, r32 and r32[0], r64[0], dtype, "from_noise z")
    check(lp, r32 and r32[1], r64[1], dtype, "from_noise log_p")
    assert torch.equal(z2, z) and torch.equal(lp2, lp)
    print("%s %s %s max |log_prob(z) - log_p| %.3e" % (family, case, dtype, float((back - lp).abs().max())))
    check(back, r32 and r32[1], r64[1], dtype, "log_prob(z) of the returned z")
    for zz, ll, n in ((zf, lf, 33), (zn, ln, b)):
        assert zz.shape == (n,) + eps.shape[1:] and ll.shape == (n,) and zz.dtype == dtype
        assert torch.isfinite(zz).all() and torch.isfinite(ll).all()


# ---------------------------------------------------------------- 3. / 4. gradients
def _weights(b):
    return torch.linspace(0.5, 1.5, b, dtype=torch.float64)


def _ref_grads(family, direction, dtype, p, x, gamma, w):
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    p = {k: leaf(v) for k, v in p.items()}
    x = leaf(x)
    out = {}
    if direction == "log_prob":
        loss = (ref.log_prob(family, x, p) * w.to(dtype)).sum()
    else:
        gamma = leaf(gamma)
        z, lp = ref.sample(family, x, gamma, p)
        loss = (lp * w.to(dtype)).sum() + 1e-3 * (z * z).sum()
    loss.backward()
    out["input"] = x.grad
    if direction == "sample":
        out["log_gamma"] = gamma.grad * gamma.detach()
    out.update({k: v.grad for k, v in p.items()})
    return out


def _hip_grads(q, direction, x, gamma, w):
    q.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    out = {}
    if direction == "log_prob":
        loss = (q.log_prob(x) * w).sum()
    else:
        gamma = gamma.clone().requires_grad_()
        z, lp = q.from_noise(x, gamma)
        loss = (lp * w).sum() + 1e-3 * (z * z).sum()
    loss.backward()
    out["input"] = x.grad
    if direction == "sample":
        # compared as the gradient with respect to log gamma: gamma reaches 1e-13 and below, the raw one has no scale
        out["log_gamma"] = gamma.grad * gamma.detach()
    out.update({k: v.grad for k, v in q.named_parameters()})
    return {k: (None if v is None else v.clone()) for k, v in out.items()}


@functools.lru_cache(maxsize=8)
def gradient_reference(family, shape, b, direction, dtype):
    """(fp32 or None, fp64) autograd gradients of the restatement; computed once for the tests that share a case."""
    p, eps, gamma, z = ref.inputs(family, shape, b)
    x = eps if direction == "sample" else z
    p, x, gamma = cast(p, dtype), x.to(dtype), gamma.to(dtype)
    r64 = _ref_grads(family, direction, torch.float64, p, x, gamma, _weights(b))
    r32 = _ref_grads(family, direction, torch.float32, p, x, gamma, _weights(b)) if dtype == torch.float32 else None
    for r in (r64, r32):
        assert r is None or all(torch.isfinite(v).all() for v in r.values()), "the reference gradient is not finite"
    return r32, r64


def _compare_grads(got, r32, r64, dtype, what=""):
    for k in sorted(r64):
        assert got[k] is not None and got[k].dtype == dtype and got[k].shape == r64[k].shape, k
        print("%s d/d%s max |got - fp64 reference| %.3e of %.3e" % (
            what, k, float((got[k].cpu().double() - r64[k]).abs().max()), float(r64[k].abs().max())))
    for k in sorted(r64):
        check(got[k], r32 and r32[k], r64[k], dtype, "d/d" + k)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("direction", ["log_prob", "sample"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_gradients_match_autograd_on_the_restatement(hip, family, case, direction, dtype):
    """Loss sum_b w_b log_p_b, w = linspace(0.5, 1.5, B), plus 1e-3 sum z^2 through from_noise: gradients with respect to
    z (eps and log gamma when sampling), loc, log_scale and the tail parameter.  Two backward passes: equal bits."""
    shape, b = case
    p, eps, gamma, z = ref.inputs(family, shape, b)
    r32, r64 = gradient_reference(family, shape, b, direction, dtype)
    q = build(family, shape, p, dtype)
    x = cuda(eps if direction == "sample" else z, dtype)
    args = (direction, x, cuda(gamma, dtype), cuda(_weights(b), dtype))
    got, again = _hip_grads(q, *args), _hip_grads(q, *args)
    assert sorted(got) == sorted(r64)
    for k in got:
        assert torch.equal(got[k], again[k]), "gradient of %s differs between two backward passes" % k
    assert _lib.lib().vcnf_tail_bwd_groups(b, q.d) >= 1
    _compare_grads(got, r32, r64, dtype, "%s %s %s %s" % (family, case, direction, dtype))
    # trainable=False: no parameter gradients (the dz-only launch), and the input gradient keeps its bits
    frozen = build(family, shape, p, dtype, trainable=False)
    cold = _hip_grads(frozen, *args)
    assert sorted(cold) == sorted(k for k in got if k in ("input", "log_gamma")) and not list(frozen.parameters())
    assert all(t.grad is None for t in frozen.buffers())
    assert torch.equal(cold["input"], got["input"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [(7, 63), (64, B), (257, B)], ids=case_id)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_log_prob_vjp_adds_the_incoming_gradient(hip, family, case, dtype):
    """vcnf_tail_log_prob_bwd_* with gz_in: dz = gz_in + g dlogp/dz, the parameter sums unchanged."""
    shape, b = case
    p, eps, _, z = ref.inputs(family, shape, b)
    r32, r64 = gradient_reference(family, shape, b, "log_prob", dtype)
    q = build(family, shape, p, dtype)
    zc, w, gz = cuda(z, dtype), cuda(_weights(b), dtype), cuda(eps, dtype)
    loc, ls, tail, _ = rows(q)
    with torch.no_grad():
        plain = _lib.tail_log_prob_bwd(zc, loc, ls, tail, FAMILY_ID[family], w)
        added = _lib.tail_log_prob_bwd(zc, loc, ls, tail, FAMILY_ID[family], w, gz_in=gz)
        only = _lib.tail_log_prob_bwd(zc, loc, ls, tail, FAMILY_ID[family], w, gz_in=gz, rows=False)
    want64 = r64["input"] + cast(eps, dtype).double()
    want32 = r32["input"] + eps.float() if dtype == torch.float32 else None
    check(added[0], want32, want64, dtype, "dz with gz_in")
    check(plain[0], r32 and r32["input"], r64["input"], dtype, "dz")
    assert torch.equal(only[0], added[0]) and only[1:] == (None, None, None)
    for a, c in zip(plain[1:], added[1:]):
        assert torch.equal(a, c)


# ---------------------------------------------------------------- 5. exact zeros
def _zero_case(family, value, dtype):
    g = torch.Generator().manual_seed(ref.seed_of("zeros", family, value))
    p = {"loc": torch.randn(1, 3, generator=g, dtype=torch.float64), "log_scale": 0.3 * torch.randn(1, 3, generator=g, dtype=torch.float64),
         ref.TAIL[family]: torch.full((1, 3), math.log(value), dtype=torch.float64)}
    p = cast(p, dtype)
    return p, p["loc"].expand(2, 3).clone(), torch.tensor([0.75, 1.5], dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family,value", [("gen_gaussian", 1.0), ("gen_gaussian", 1.5), ("gen_gaussian", 2.0), ("student_t", 3.0)])
def test_gradients_at_u_equal_zero_match_autograd(hip, family, value, dtype):
    p, z, w = _zero_case(family, value, dtype)
    r64 = _ref_grads(family, "log_prob", torch.float64, p, z, None, w)
    r32 = _ref_grads(family, "log_prob", torch.float32, p, z, None, w) if dtype == torch.float32 else None
    assert all(torch.isfinite(v).all() for v in r64.values())
    got = _hip_grads(build(family, 3, p, dtype), "log_prob", z.cuda(), None, w.cuda())
    _compare_grads(got, r32, r64, dtype, "%s %g at u = 0" % (family, value))
    assert float(got["input"].abs().max()) == 0.0 and float(got["loc"].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gradients_at_u_equal_zero_below_beta_one_follow_the_convention(hip, dtype):
    """beta = 0.7, z == loc: torch's autograd on the restatement gives NaN (0 x inf); the kernel gives dz = 0, d_loc = 0,
    d_log_scale = -sum_b g_b and a tail-parameter gradient that is the normaliser's term alone,
    sum_b g_b dc/dlog_beta.  The last is compared with torch's fp64 derivative of the restatement's normaliser: to
    rtol 1e-10 in fp64; in fp32 the module rounds that fp64 derivative once and adds an exact zero, and the two-term sum
    of g rounds once more: rtol 1e-6."""
    family = "gen_gaussian"
    p, z, w = _zero_case(family, 0.7, dtype)
    naive = _ref_grads(family, "log_prob", torch.float64, p, z, None, w)
    assert torch.isnan(naive["input"]).all(), "the restatement's autograd is expected to fail here"
    got = _hip_grads(build(family, 3, p, dtype), "log_prob", z.cuda(), None, w.cuda())
    assert all(torch.isfinite(v).all() for v in got.values())
    assert float(got["input"].abs().max()) == 0.0 and float(got["loc"].abs().max()) == 0.0
    total = float(w.double().sum())
    assert_close(got["log_scale"], torch.full((1, 3), -total, dtype=torch.float64), rtol=1e-6 if dtype == torch.float32 else 1e-15,
                 atol=0, what="d/dlog_scale")
    log_beta = p["log_beta"].double().clone().requires_grad_()
    (total * ref.normaliser(family, log_beta)).sum().backward()
    assert_close(got["log_beta"], log_beta.grad, rtol=1e-6 if dtype == torch.float32 else 1e-10, atol=0, what="d/dlog_beta")


# ---------------------------------------------------------------- 7. the drawn distribution
DRAWN = {"student_t": (1.5, 3.0, 8.0, 30.0), "gen_gaussian": (0.6, 1.0, 2.0, 2.5)}
LOG_SCALE = (-0.5, 0.0, 0.3, 1.0)


def _entropy(family):
    t = torch.tensor(DRAWN[family], dtype=torch.float64)
    ls = torch.tensor(LOG_SCALE, dtype=torch.float64)
    if family == "student_t":
        h = (0.5 * (t + 1) * (torch.digamma(0.5 * (t + 1)) - torch.digamma(0.5 * t)) + 0.5 * torch.log(t) + torch.lgamma(0.5 * t)
             + math.lgamma(0.5) - torch.lgamma(0.5 * (t + 1)) + ls)
    else:
        h = 1.0 / t - torch.log(t) + math.log(2.0) + torch.lgamma(1.0 / t) + ls
    return float(h.sum())


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_forward_draws_the_stated_distribution(hip, family, seed=11):
    """65 536 draws at D = 4: the mean of the returned log p is minus the closed-form entropy within 5 standard errors
    (taken from the sample).  A gamma concentration of nu for nu / 2, or 2 / beta for 1 / beta, is off by hundreds."""
    n = 65536
    kw = {"df": DRAWN[family]} if family == "student_t" else {"beta": DRAWN[family]}
    q = getattr(nf.distributions, CLASSES[family])(4, **kw)
    with torch.no_grad():
        q.log_scale.copy_(torch.tensor([LOG_SCALE]))
    q = q.cuda()
    torch.manual_seed(seed)
    with torch.no_grad():
        z, lp = q(n)
    assert z.shape == (n, 4) and lp.shape == (n,) and torch.isfinite(z).all() and torch.isfinite(lp).all()
    lp = lp.double().cpu()
    se = float(lp.std()) / math.sqrt(n)
    off = (float(lp.mean()) + _entropy(family)) / se
    print("%s seed %d: mean log p %.5f, -entropy %.5f, %.2f standard errors apart" % (family, seed, float(lp.mean()), -_entropy(family), off))
    assert abs(off) <= 5.0


# ---------------------------------------------------------------- 8. in a flow
def _flow(family, dtype, seed=41):
    torch.manual_seed(seed)
    flows = [nf.flows.CoupledRationalQuadraticSpline(8, 1, 16, reverse_mask=bool(i)) for i in range(2)]
    p = ref.inputs(family, 8, 256)[0]
    q0 = getattr(nf.distributions, CLASSES[family])(8)
    q0.load_state_dict(cast(p, torch.float32))
    return nf.NormalizingFlow(q0, flows).to(dtype).cuda(), cast(cast(p, torch.float32), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_flow_log_prob_and_objectives(hip, family, dtype):
    """Two CoupledRationalQuadraticSpline(8, 1, 16) over the base, B = 256.  log_prob(x) against the layers walked by hand
    plus the restated base term; forward_kld and reverse_kld (against a fixed DiagGaussian) run backward and reach loc,
    log_scale and the tail parameter with finite, non-zero gradients."""
    n = 256
    model, p = _flow(family, dtype)
    model.eval()
    g = torch.Generator().manual_seed(43)
    x = (1.5 * torch.randn(n, 8, generator=g, dtype=torch.float64)).to(dtype)
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
    for name, par in model.q0.named_parameters():
        assert par.grad is not None and torch.isfinite(par.grad).all() and float(par.grad.abs().sum()) > 0, name
    model.zero_grad(set_to_none=True)
    model.p = nf.distributions.DiagGaussian(8, trainable=False).to(dtype).cuda()
    torch.manual_seed(3)
    loss = model.reverse_kld(256)
    loss.backward()
    assert torch.isfinite(loss)
    for name, par in model.named_parameters():
        assert par.grad is not None and torch.isfinite(par.grad).all(), name
    for name, par in model.q0.named_parameters():
        assert float(par.grad.abs().sum()) > 0, name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("family", ref.FAMILIES)
def test_tail_parameter_gradient_includes_the_path_through_gamma(hip, family, dtype):
    """forward(n) draws gamma with autograd on.  With the same draws supplied as constants the tail parameter's gradient
    lacks sum_b dgamma dgamma/dconcentration dconcentration/dlog_tail, torch's implicit derivative of its gamma sampler;
    the two differ by exactly that term.  Sums of n = 256 terms in the module's dtype: 1e-4 / 1e-10 of the largest entry."""
    n = 256
    p = ref.inputs(family, 8, 256)[0]
    q = build(family, 8, p, dtype)
    tail = ref.TAIL[family]
    loss = lambda z, lp: lp.sum() + 0.1 * (z * z).sum()

    torch.manual_seed(5)
    z, lp = q(n)
    loss(z, lp).backward()
    full = getattr(q, tail).grad.clone()
    q.zero_grad(set_to_none=True)

    torch.manual_seed(5)
    eps = torch.randn(n, 8, dtype=dtype, device="cuda")
    conc = q._rows()[4].detach().expand(n, 8)
    gamma = torch._standard_gamma(conc).requires_grad_()
    z2, lp2 = q.from_noise(eps, gamma)
    assert torch.equal(z2, z) and torch.equal(lp2, lp)
    loss(z2, lp2).backward()
    cut = getattr(q, tail).grad.clone()
    dconc = conc[0] if family == "student_t" else -conc[0]          # d(nu / 2)/dlog nu = nu / 2, d(1 / beta)/dlog beta = -1 / beta
    path = (gamma.grad * torch._standard_gamma_grad(conc, gamma.detach())).sum(0) * dconc
    assert torch.isfinite(full).all() and float(path.abs().max()) > 0
    scale = float(full.abs().max())
    assert_close(full.reshape(-1), (cut.reshape(-1) + path).cpu(), rtol=0, atol=(1e-4 if dtype == torch.float32 else 1e-10) * scale,
                 what="d/d" + tail)
    assert float((full - cut).abs().max()) > 1e-3 * scale, "the gamma path contributes nothing"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_multiscale_level_with_a_student_t_base(hip, dtype):
    """One MultiscaleFlow(class_cond=False) level: Squeeze over StudentT((4, 2, 2)); log_prob against the restatement."""
    p = ref.inputs("student_t", (4, 2, 2), 64)[0]
    q0 = build("student_t", (4, 2, 2), p, dtype)
    model = nf.MultiscaleFlow([q0], [[nf.flows.Squeeze()]], [], class_cond=False).cuda()
    g = torch.Generator().manual_seed(7)
    x = (2.0 * torch.randn(64, 1, 4, 4, generator=g, dtype=torch.float64)).to(dtype)
    with torch.no_grad():
        lp = model.log_prob(x.cuda())
        z, _ = model.flows[0][0].inverse(x.cuda())
    assert z.shape == (64, 4, 2, 2)
    r32, r64 = references(lambda z_, p_: ref.log_prob("student_t", z_, p_), dtype, z.cpu(), p)
    check(lp, r32, r64, dtype, "MultiscaleFlow.log_prob")
