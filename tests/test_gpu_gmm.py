"""GaussianMixture base distribution on the HIP kernels (csrc/gaussian_mixture.hip).

The reference is the plain-torch restatement below of normflow 1.2's GaussianMixture arithmetic, run on the CPU in fp32
and in fp64 on the inputs as the module sees them.  fp32 results are judged by helpers.parity (against the
restatement's fp32 run, with its own fp32-vs-fp64 error as the yardstick); fp64 results by rtol = atol = 1e-10, the
figure the fp64 Gaussian tests use.  Inputs are seeded: loc ~ 2 N(0, 1), log_scale ~ 0.3 N(0, 1), weight_scores ~
N(0, 1), z drawn from the mixture itself (B = 4096) and the first B / 8 rows multiplied by 25 (far tails: a naive
log(sum(exp)) is -inf there).  Before anything is compared the test checks that the restatement is finite in both
precisions, that every mode is drawn and that every mode is the arg-max of some row."""
import functools
import math
import zlib

import pytest
import torch

import vcnf_amd as nf
from helpers import assert_close, parity

pytestmark = pytest.mark.gpu

B = 4096
SHAPES = [(1, 1), (3, 2), (5, 7), (16, 64), (64, 30), (10, 257)]
# the edges of the supported range M D <= 8192: tables of 128 KiB and more in fp64, the per-mode constant outside LDS
# (8192, 1), LDS filled to the last byte (4096, 2), rows too long for a lane group's registers (1, 8192)
EDGE_SHAPES = [(8192, 1), (4096, 2), (1, 8192), (2, 4096)]
F64 = dict(rtol=1e-10, atol=1e-10)
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]


# ---------------------------------------------------------------- the restatement (any dtype, any device)
def ref_log_prob(z, p):
    """p: loc, log_scale [1, M, D], weight_scores [1, M]"""
    w = torch.softmax(p["weight_scores"], 1)
    u = (z[:, None, :] - p["loc"]) / torch.exp(p["log_scale"])
    a = -0.5 * z.shape[1] * math.log(2 * math.pi) + torch.log(w) - 0.5 * torch.sum(u ** 2, 2) - torch.sum(p["log_scale"], 2)
    return torch.logsumexp(a, 1)


def ref_modes(z, p):
    u = (z[:, None, :] - p["loc"]) / torch.exp(p["log_scale"])
    a = torch.log_softmax(p["weight_scores"], 1) - 0.5 * torch.sum(u ** 2, 2) - torch.sum(p["log_scale"], 2)
    return a.argmax(1)


def ref_sample(eps, mode, p):
    z = eps * torch.exp(p["log_scale"][0, mode]) + p["loc"][0, mode]
    return z, ref_log_prob(z, p)


# ---------------------------------------------------------------- seeded inputs, one set per shape
def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def cast(t, dtype):
    if isinstance(t, dict):
        return {k: cast(v, dtype) for k, v in t.items()}
    return t.to(dtype) if t.is_floating_point() else t


@functools.lru_cache(maxsize=None)
def inputs(m, d, b=B, tails=True):
    """(params, mode, eps, z) in fp64; z = the mixture's own draw, the first b // 8 rows x 25 with ``tails``."""
    g = torch.Generator().manual_seed(seed_of("gmm", m, d))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    p = {"loc": 2.0 * r(1, m, d), "log_scale": 0.3 * r(1, m, d), "weight_scores": r(1, m)}
    mode = torch.multinomial(torch.softmax(p["weight_scores"], 1)[0], b, replacement=True, generator=g)
    eps = r(b, d)
    z, _ = ref_sample(eps, mode, p)
    if tails:
        z = z.clone()
        z[: b // 8] *= 25.0
    return p, mode, eps, z


def references(fn, dtype, *tensors):
    """fn on the CPU: (fp32 run or None, fp64 run) of the inputs rounded to ``dtype``; every output finite."""
    seen = [cast(t, dtype) for t in tensors]
    r64 = fn(*[cast(t, torch.float64) for t in seen])
    r32 = fn(*[cast(t, torch.float32) for t in seen]) if dtype == torch.float32 else None
    for r in (r64, r32):
        for t in ((r if isinstance(r, tuple) else (r,)) if r is not None else ()):
            assert torch.isfinite(t).all(), "the reference output is not finite"
    return r32, r64


def check(got, r32, r64, dtype, what):
    if dtype == torch.float32:
        parity(got, r32, r64, what=what)
    else:
        assert got.dtype == torch.float64
        assert_close(got, r64, what=what, **F64)


def build(m, d, p, dtype, trainable=True):
    q = nf.distributions.GaussianMixture(m, d, trainable=trainable).to(dtype)
    q.load_state_dict(cast(p, dtype))
    return q.cuda()


def cuda(t, dtype):
    return cast(t, dtype).cuda()


def check_inputs(m, d, p, mode, z):
    """The conditions under which the comparison means something (the references' finiteness is checked where they
    are computed)."""
    assert len(torch.unique(mode)) == m, "a mode is never drawn"
    assert len(torch.unique(ref_modes(z, p))) == m, "a mode is never the arg-max"


# ---------------------------------------------------------------- 1. log_prob
def _log_prob_case(m, d, dtype, b=B):
    p, mode, _, z = inputs(m, d, b)
    if b == B:
        check_inputs(m, d, p, mode, z)
    r32, r64 = references(ref_log_prob, dtype, z, p)
    q = build(m, d, p, dtype)
    zc = cuda(z, dtype)
    with torch.no_grad():
        lp = q.log_prob(zc)
        acc = torch.full((b,), 2.0, dtype=dtype, device="cuda")
        assert q.log_prob(zc, out=acc) is acc
        again = q.log_prob(zc)
    assert lp.shape == (b,) and lp.dtype == dtype
    check(lp, r32, r64, dtype, "log_prob")
    # accumulation into an existing buffer: one more rounding of 2 + log_p
    assert_close(acc, 2.0 + lp.double().cpu(), rtol=2e-7 if dtype == torch.float32 else 1e-15, atol=0, what="log_prob(out=)")
    assert torch.equal(again, lp), "the same call twice gives different bits"
    return lp, r64


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_log_prob(hip, shape, dtype):
    lp, r64 = _log_prob_case(*shape, dtype)
    # exp(a) underflows below -745 even in fp64: there a naive log(sum(exp(a))) gives -inf
    assert bool((r64 < -745.0).any()), "no row is in the far tail"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("b", [1, 63, 64, 65, 1000])
def test_log_prob_batch_sizes(hip, b, dtype):
    _log_prob_case(5, 7, dtype, b)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=str)
def test_log_prob_and_gradients_at_the_edge_of_the_range(hip, shape, dtype):
    m, d = shape
    _log_prob_case(m, d, dtype, 256)
    _gradient_case(m, d, "log_prob", dtype, 256)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [1, 64])
def test_one_mode_agrees_with_diag_gaussian(hip, d, dtype):
    """M = 1: the mixture is the DiagGaussian with the same loc / log_scale; to the parity tolerance, not bitwise."""
    p, _, _, z = inputs(1, d)
    q = build(1, d, p, dtype)
    dg = nf.distributions.DiagGaussian(d).to(dtype)
    dg.load_state_dict({"loc": cast(p["loc"][0], dtype), "log_scale": cast(p["log_scale"][0], dtype)})
    dg = dg.cuda()
    _, r64 = references(ref_log_prob, dtype, z, p)
    with torch.no_grad():
        got, want = q.log_prob(cuda(z, dtype)), dg.log_prob(cuda(z, dtype))
    check(got, want.cpu(), r64 if dtype == torch.float32 else want.cpu(), dtype, "GaussianMixture(1, d) vs DiagGaussian")


# ---------------------------------------------------------------- 2. from_noise / forward
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_from_noise(hip, shape, dtype):
    m, d = shape
    p, mode, eps, _ = inputs(m, d)
    r32, r64 = references(lambda e, p_: ref_sample(e, mode, p_), dtype, eps, p)
    q = build(m, d, p, dtype)
    with torch.no_grad():
        z, lp = q.from_noise(cuda(eps, dtype), mode.cuda())
        z2, lp2 = q.from_noise(cuda(eps, dtype), mode.cuda())
        back = q.log_prob(z)
        zf, lf = q(33)
    assert z.shape == (B, d) and lp.shape == (B,) and z.dtype == dtype
    check(z, r32 and r32[0], r64[0], dtype, "from_noise z")
    check(lp, r32 and r32[1], r64[1], dtype, "from_noise log_p")
    assert torch.equal(z2, z) and torch.equal(lp2, lp)
    # bitwise: the sampling launch evaluates the density of the z it stores with the code of log_prob
    assert torch.equal(back, lp), "log_prob(z) of the returned z differs from the returned log_p"
    assert zf.shape == (33, d) and lf.shape == (33,) and zf.dtype == dtype
    assert torch.isfinite(zf).all() and torch.isfinite(lf).all()


def test_forward_draws_the_modes_by_their_weights(hip):
    """65 536 draws, weights (0.6, 0.3, 0.1), unit scales, modes 10 apart: a sample's mode is its nearest loc.  The
    share's standard deviation is sqrt(p (1 - p) / n) <= 0.0019, so 0.01 is more than 5 sigma for every mode."""
    loc = [[-10.0, 0.0], [0.0, 10.0], [10.0, 0.0]]
    weights = [0.6, 0.3, 0.1]
    q = nf.distributions.GaussianMixture(3, 2, loc=loc, weights=weights).cuda()
    torch.manual_seed(7)
    with torch.no_grad():
        z, lp = q(65536)
    assert z.shape == (65536, 2) and lp.shape == (65536,) and torch.isfinite(lp).all()
    nearest = torch.cdist(z.cpu().double(), torch.tensor(loc, dtype=torch.float64)).argmin(1)
    share = torch.bincount(nearest, minlength=3).double() / 65536
    print("mode shares", share.tolist())
    assert float((share - torch.tensor(weights, dtype=torch.float64)).abs().max()) <= 0.01


# ---------------------------------------------------------------- 3. modes outside the table
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(5, 7), (16, 64), (10, 257)], ids=str)
def test_out_of_range_modes_give_nan_for_those_samples_only(hip, shape, dtype):
    m, d = shape
    p, mode, eps, _ = inputs(m, d)
    q = build(m, d, p, dtype)
    bad = torch.zeros(B, dtype=torch.bool)
    mode_bad = mode.clone()
    mode_bad[5], mode_bad[B - 3] = m, -1
    bad[5] = bad[B - 3] = True
    bad = bad.cuda()
    with torch.no_grad():
        z, lp = q.from_noise(cuda(eps, dtype), mode.cuda())
        zb, lpb = q.from_noise(cuda(eps, dtype), mode_bad.cuda())
    for clean, dirty in ((z, zb), (lp, lpb)):
        nan = torch.isnan(dirty.reshape(B, -1))
        assert not torch.isnan(clean).any()
        assert torch.equal(nan.all(1), bad) and torch.equal(nan.any(1), bad)
        assert torch.equal(dirty[~bad], clean[~bad])


# ---------------------------------------------------------------- 4. gradients
def _ref_grads(direction, dtype, p, mode, x, w, gz):
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    p = {k: leaf(v) for k, v in p.items()}
    x = leaf(x)
    if direction == "log_prob":
        loss = (ref_log_prob(x, p) * w.to(dtype)).sum()
    else:
        z, lp = ref_sample(x, mode, p)
        loss = (lp * w.to(dtype)).sum() + (z * gz.to(dtype)).sum()
    loss.backward()
    out = {"input": x.grad}
    out.update({k: v.grad for k, v in p.items()})
    assert all(torch.isfinite(v).all() for v in out.values())
    return out


def _hip_grads(q, direction, mode, x, w, gz):
    q.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    if direction == "log_prob":
        loss = (q.log_prob(x) * w).sum()
    else:
        z, lp = q.from_noise(x, mode)
        loss = (lp * w).sum() + (z * gz).sum()
    loss.backward()
    out = {"input": x.grad}
    out.update({k: v.grad for k, v in q.named_parameters()})
    return {k: (None if v is None else v.clone()) for k, v in out.items()}


def _compare_grads(got, r32, r64, dtype):
    for k in sorted(r64):
        assert got[k] is not None and got[k].dtype == dtype and got[k].shape == r64[k].shape, k
        if dtype == torch.float32:
            parity(got[k], r32[k], r64[k], what="d/d" + k)
        else:
            assert_close(got[k], r64[k], rtol=1e-9, atol=1e-9 * float(r64[k].abs().max()), what="d/d" + k)


def _gradient_case(m, d, direction, dtype, b=B):
    """Loss sum(w log_p), plus sum(gz z) for sampling, unit-scale random cotangents; the draws without the x 25 rows."""
    p, mode, eps, z = inputs(m, d, b, tails=False)
    g = torch.Generator().manual_seed(seed_of("cot", m, d))
    w = torch.randn(b, generator=g, dtype=torch.float64)
    gz = torch.randn(b, d, generator=g, dtype=torch.float64)
    x = eps if direction == "sample" else z
    p, x, w, gz = cast(p, dtype), x.to(dtype), w.to(dtype), gz.to(dtype)
    r64 = _ref_grads(direction, torch.float64, p, mode, x, w, gz)
    r32 = _ref_grads(direction, torch.float32, p, mode, x, w, gz) if dtype == torch.float32 else None
    q = build(m, d, p, dtype)
    args = (q, direction, mode.cuda(), x.cuda(), w.cuda(), gz.cuda())
    got, again = _hip_grads(*args), _hip_grads(*args)
    assert sorted(got) == sorted(r64)
    for k in got:
        assert torch.equal(got[k], again[k]), "gradient of %s differs between two backward passes" % k
    _compare_grads(got, r32, r64, dtype)
    return q, args, got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("direction", ["log_prob", "sample"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradients_match_autograd_on_the_restatement(hip, shape, direction, dtype):
    """Gradients with respect to z / eps, loc, log_scale and weight_scores.  fp32: helpers.parity against the
    restatement's fp32 and fp64 autograd.  fp64: rtol 1e-9 and, a parameter gradient being a sum over the batch of terms
    that cancel, an absolute tolerance of 1e-9 x the largest entry of that gradient.  Two backward passes: equal bits."""
    m, d = shape
    _, args, got = _gradient_case(m, d, direction, dtype)
    # trainable=False: no parameter gradients, and the input gradient keeps its bits
    p = inputs(m, d, B, False)[0]
    frozen = build(m, d, cast(p, dtype), dtype, trainable=False)
    cold = _hip_grads(frozen, *args[1:])
    assert sorted(cold) == ["input"] and not list(frozen.parameters())
    assert all(t.grad is None for t in frozen.buffers())
    assert torch.equal(cold["input"], got["input"])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_far_tail_row_has_a_finite_matching_input_gradient(hip, dtype):
    """One row 25 x out: the responsibilities saturate to one mode, dz stays finite and matches the restatement."""
    m, d = 5, 7
    p, mode, _, z = inputs(m, d)
    p, row = cast(p, dtype), z[:1].to(dtype)
    w, none = torch.ones(1, dtype=dtype), torch.zeros(1, d, dtype=dtype)
    r64 = _ref_grads("log_prob", torch.float64, p, mode[:1], row, w, none)
    r32 = _ref_grads("log_prob", torch.float32, p, mode[:1], row, w, none) if dtype == torch.float32 else None
    resp = torch.softmax(torch.log_softmax(p["weight_scores"].double(), 1) - 0.5 * (((row.double()[:, None] - p["loc"].double()) /
                         torch.exp(p["log_scale"].double())) ** 2).sum(2) - p["log_scale"].double().sum(2), 1)
    assert float(resp.max()) > 1.0 - 1e-12, "the row is not in the far tail"
    got = _hip_grads(build(m, d, p, dtype), "log_prob", None, row.cuda(), w.cuda(), None)
    assert torch.isfinite(got["input"]).all()
    _compare_grads(got, r32, r64, dtype)


# ---------------------------------------------------------------- 5. in a flow
def _flow(dtype, seed=41):
    torch.manual_seed(seed)
    flows = []
    for _ in range(4):
        flows += [nf.flows.AffineCouplingBlock(nf.nets.MLP([1, 16, 16, 2], init_zeros=False)), nf.flows.Permute(2, mode="swap")]
    p = inputs(4, 2)[0]
    q0 = nf.distributions.GaussianMixture(4, 2)
    q0.load_state_dict(cast(p, torch.float32))
    model = nf.NormalizingFlow(q0, flows).to(dtype).cuda()
    return model, cast(cast(p, torch.float32), dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_flow_log_prob_sampling_and_objectives(hip, dtype):
    """[AffineCouplingBlock(MLP), Permute] x 4 over GaussianMixture(4, 2), B = 1024.  log_prob(x) against the layers'
    plain inverse chain plus the restated base term; sample_from then log_prob reproduces log q to 1e-4 (fp32) / 1e-10
    (fp64) relative to 1 + |log q|, the figures of the class-conditional flow test; forward_kld = -mean of the reference;
    reverse_kld runs backward and reaches every parameter of the base."""
    n = 1024
    model, p = _flow(dtype)
    model.eval()
    g = torch.Generator().manual_seed(43)
    x = torch.randn(n, 2, generator=g, dtype=torch.float64).to(dtype)
    with torch.no_grad():
        lp = model.log_prob(x.cuda())
        z, log_det = x.cuda(), torch.zeros(n, dtype=dtype, device="cuda")
        for flow in reversed(model.flows):
            z, ld = flow.inverse(z)
            log_det = log_det + ld
    z, log_det = z.cpu(), log_det.cpu()
    want = {dt: log_det.to(dt) + ref_log_prob(z.to(dt), cast(p, dt)) for dt in (torch.float32, torch.float64)}
    assert all(torch.isfinite(v).all() for v in want.values())
    check(lp, want[torch.float32], want[torch.float64], dtype, "NormalizingFlow.log_prob")
    eps = torch.randn(n, 2, generator=g, dtype=torch.float64).to(dtype).cuda()
    with torch.no_grad():
        zs, lq = model.sample_from(eps)
        back = model.log_prob(zs)
        z1, l1 = model.sample(17)
    tol = 1e-4 if dtype == torch.float32 else 1e-10
    assert torch.isfinite(lq).all() and float(((back - lq).abs() / (1.0 + lq.abs())).max()) <= tol
    assert z1.shape == (17, 2) and l1.shape == (17,) and torch.isfinite(l1).all()
    model.train()
    loss = model.forward_kld(x.cuda())
    loss.backward()
    assert_close(loss, -want[torch.float64].mean(), rtol=1e-5 if dtype == torch.float32 else 1e-10,
                 atol=1e-5 if dtype == torch.float32 else 1e-10, what="forward_kld")
    for name, par in model.named_parameters():
        assert par.grad is not None and torch.isfinite(par.grad).all(), name
    model.zero_grad(set_to_none=True)
    model.p = nf.distributions.DiagGaussian(2, trainable=False).to(dtype).cuda()
    torch.manual_seed(3)
    loss = model.reverse_kld(256)
    loss.backward()
    assert torch.isfinite(loss)
    for name, par in model.q0.named_parameters():
        assert par.grad is not None and torch.isfinite(par.grad).all() and float(par.grad.abs().sum()) > 0, name


def test_flow_trains_on_two_clusters(hip):
    """50 Adam steps (lr 1e-2) of forward_kld on seeded two-cluster data: the loss ends lower than it started and every
    parameter of the base has moved."""
    model, _ = _flow(torch.float32)
    model.train()
    g = torch.Generator().manual_seed(47)
    centre = torch.tensor([[-2.0, 1.0], [2.0, -1.0]])[torch.randint(2, (1024,), generator=g)]
    x = (centre + 0.4 * torch.randn(1024, 2, generator=g)).cuda()
    before = {k: v.detach().clone() for k, v in model.q0.named_parameters()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    losses = []
    for _ in range(50):
        opt.zero_grad()
        loss = model.forward_kld(x)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float(model.forward_kld(x))
    print("GaussianMixture flow forward_kld: %.4f -> %.4f" % (losses[0], final))
    assert all(math.isfinite(v) for v in losses) and final < losses[0], losses
    for k, v in model.q0.named_parameters():
        assert not torch.equal(v.detach(), before[k]), "%s has not moved" % k


def test_flow_save_load(hip, tmp_path):
    model, _ = _flow(torch.float32)
    twin, _ = _flow(torch.float32, seed=45)
    with torch.no_grad():
        for par in twin.q0.parameters():
            par.add_(0.25)
    path = str(tmp_path / "gmm_flow.pt")
    model.save(path)
    twin.load(path)
    x = torch.randn(64, 2, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        assert torch.equal(model.eval().log_prob(x), twin.eval().log_prob(x))


# ---------------------------------------------------------------- 6. graph capture
def test_flow_log_prob_is_capturable(hip):
    """NormalizingFlow.log_prob(x_static) over the mixture base under torch.cuda.graph (one stream, side-stream
    warm-up): new inputs copied into the static buffer, the replay equals the eager result bitwise."""
    model, _ = _flow(torch.float32)
    model.eval()
    n = 512
    g = torch.Generator().manual_seed(9)
    draw = lambda: torch.randn(n, 2, generator=g).cuda()
    x_static = draw()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            model.log_prob(x_static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = model.log_prob(x_static)
    for _ in range(2):
        x = draw()
        x_static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = model.log_prob(x)
        assert torch.isfinite(eager).all() and torch.equal(out, eager)
