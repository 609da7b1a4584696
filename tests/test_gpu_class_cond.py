"""Class-conditional bases on the HIP kernels (csrc/class_cond_gaussian.hip): GlowBase, ClassCondDiagGaussian,
ClassCondFlow and MultiscaleFlow(class_cond=True).

The reference is the plain-torch restatement below of normflow 1.2's arithmetic (distributions/base.py:715-869), run on
the CPU in fp32 and in fp64.  fp32 results are judged by helpers.parity (noise-aware: against the restatement's fp32
run, with its own fp32-vs-fp64 error as the yardstick); fp64 results by rtol = atol = 1e-10, the figure
test_gpu_f64.py uses for the Gaussian.  Inputs are seeded, parameters N(0, 0.3^2) so that exp(log_scale) stays well
inside fp32 range, B = 4096, 10 classes; every reference output is checked to be finite and every class to occur."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vcnf_amd as nf
from helpers import assert_close, parity, fixture, glow_state

pytestmark = pytest.mark.gpu

B, NC = 4096, 10
GLOW_SHAPES = [(48, 4, 4), (12, 8, 8), (6, 16, 16), (5, 3, 3), (7,)]
CCDG_SHAPES = [(64,), (1000,), (6, 4, 4)]
F64 = dict(rtol=1e-10, atol=1e-10)
DTYPES = [torch.float32, torch.float64]


# ---------------------------------------------------------------- the restatement (any dtype, any device)
def glow_tables(p, y, shape, factor=3.0):
    """Effective loc / log_scale of GlowBase, broadcastable to [B, *shape] (base.py:818-834)."""
    loc = p["loc"] * torch.exp(p["loc_logs"] * factor)
    ls = p["log_scale"] * torch.exp(p["log_scale_logs"] * factor)
    if "loc_cc" in p:
        if y.dim() == 1:
            y = F.one_hot(y, p["loc_cc"].shape[0]).to(loc.dtype)
        ones = (len(shape) - 1) * [1]
        loc = loc + (y @ p["loc_cc"]).view(y.size(0), shape[0], *ones)
        ls = ls + (y @ p["log_scale_cc"]).view(y.size(0), shape[0], *ones)
    return loc, ls, int(np.prod(shape[1:]))


def ccdg_tables(p, y, shape):
    """Per-sample loc / log_scale of ClassCondDiagGaussian [B, *shape] (base.py:741-757)."""
    if y.dim() == 1:
        y = F.one_hot(y, p["loc"].shape[-1]).to(p["loc"].dtype)
    perm = [len(shape)] + list(range(len(shape)))
    return (p["loc"] @ y.t()).permute(*perm), (p["log_scale"] @ y.t()).permute(*perm), 1


def ref_log_prob(z, loc, ls, pix, temperature):
    """-0.5 d log(2 pi) - P sum_c ls - 0.5 sum ((z - loc) / exp(ls))^2"""
    if temperature is not None:
        ls = ls + math.log(temperature)
    dims = list(range(1, z.dim()))
    d = z[0].numel()
    return -0.5 * d * math.log(2 * math.pi) - pix * torch.sum(ls, dim=dims) - 0.5 * torch.sum(((z - loc) / torch.exp(ls)) ** 2, dim=dims)


def ref_sample(eps, loc, ls, pix, temperature):
    """z = loc + exp(ls) eps, logp = -0.5 d log(2 pi) - P sum_c ls - 0.5 sum eps^2"""
    if temperature is not None:
        ls = ls + math.log(temperature)
    dims = list(range(1, eps.dim()))
    d = eps[0].numel()
    z = loc + torch.exp(ls) * eps
    return z, -0.5 * d * math.log(2 * math.pi) - pix * torch.sum(ls, dim=dims) - 0.5 * torch.sum(eps ** 2, dim=dims)


KINDS = {"glow": (nf.distributions.GlowBase, glow_tables), "ccdg": (nf.distributions.ClassCondDiagGaussian, ccdg_tables)}


# ---------------------------------------------------------------- seeded inputs
def seed_of(*case):
    return zlib.crc32(repr(case).encode())


def draw_params(kind, shape, nc, g):
    r = lambda *s: 0.3 * torch.randn(*s, generator=g, dtype=torch.float64)
    if kind == "ccdg":
        return {"loc": r(*shape, nc), "log_scale": r(*shape, nc)}
    per = (1, shape[0]) + (len(shape) - 1) * (1,)
    p = {k: r(*per) for k in ("loc", "loc_logs", "log_scale", "log_scale_logs")}
    if nc is not None:
        p["loc_cc"], p["log_scale_cc"] = r(nc, shape[0]), r(nc, shape[0])
    return p


def draw_labels(labels, g, b=B):
    if labels == "hard":
        y = torch.randint(NC, (b,), generator=g)
        assert len(torch.unique(y)) == NC, "a class does not occur among the labels"
        return y
    if labels == "soft":
        return torch.softmax(torch.randn(b, NC, generator=g, dtype=torch.float64), 1)
    return None


def cast(v, dtype):
    if v is None or not v.is_floating_point():
        return v
    return v.to(dtype)


def build(kind, shape, nc, params, dtype):
    q = KINDS[kind][0](shape, nc).to(dtype)
    q.load_state_dict({k: v.to(dtype) for k, v in params.items()})
    return q.cuda()


def references(fn, dtype, *tensors):
    """fn on the CPU: (fp32 run or None, fp64 run) of the inputs as the module sees them (rounded to ``dtype``)."""
    seen = [({k: cast(v, dtype) for k, v in t.items()} if isinstance(t, dict) else cast(t, dtype)) for t in tensors]
    up = lambda t, dt: {k: cast(v, dt) for k, v in t.items()} if isinstance(t, dict) else cast(t, dt)
    r64 = fn(*[up(t, torch.float64) for t in seen])
    r32 = fn(*[up(t, torch.float32) for t in seen]) if dtype == torch.float32 else None
    for r in (r64 if isinstance(r64, tuple) else (r64,)):
        assert torch.isfinite(r).all(), "the reference output is not finite"
    return r32, r64


def check(got, r32, r64, dtype, what):
    if dtype == torch.float32:
        parity(got, r32, r64, what=what)
    else:
        assert got.dtype == torch.float64
        assert_close(got, r64, what=what, **F64)


def cuda(v, dtype):
    return None if v is None else cast(v, dtype).cuda()


def _density_and_sampling(kind, shape, labels, temperature, dtype):
    g = torch.Generator().manual_seed(seed_of(kind, shape, labels))
    nc = None if labels == "none" else NC
    tables = KINDS[kind][1]
    params = draw_params(kind, shape, nc, g)
    y = draw_labels(labels, g)
    z = torch.randn(B, *shape, generator=g, dtype=torch.float64)
    q = build(kind, shape, nc, params, dtype)
    q.temperature = temperature
    lp32, lp64 = references(lambda p, y_, z_: ref_log_prob(z_, *tables(p, y_, shape), temperature), dtype, params, y, z)
    s32, s64 = references(lambda p, y_, e_: ref_sample(e_, *tables(p, y_, shape), temperature), dtype, params, y, z)
    with torch.no_grad():
        lp = q.log_prob(cuda(z, dtype), cuda(y, dtype))
        zs, lq = q.from_noise(cuda(z, dtype), cuda(y, dtype))
        acc = torch.full((B,), 2.0, dtype=dtype, device="cuda")
        assert q.log_prob(cuda(z, dtype), cuda(y, dtype), out=acc) is acc
    assert lp.shape == (B,) and zs.shape == (B,) + tuple(shape) and lq.shape == (B,)
    check(lp, lp32, lp64, dtype, "log_prob")
    check(zs, s32 and s32[0], s64[0], dtype, "from_noise z")
    check(lq, s32 and s32[1], s64[1], dtype, "from_noise logp")
    # accumulation into an existing buffer: the same density on top of what was there
    assert_close(acc - 2.0, lp.cpu(), rtol=1e-6 if dtype == torch.float32 else 1e-12, atol=1e-3 if dtype == torch.float32 else 1e-9,
                 what="log_prob(out=)")
    with torch.no_grad():                                  # the same call twice: the same bits
        assert torch.equal(q.log_prob(cuda(z, dtype), cuda(y, dtype)), lp)
        z2, lq2 = q.from_noise(cuda(z, dtype), cuda(y, dtype))
        assert torch.equal(z2, zs) and torch.equal(lq2, lq)
        zz, ll = q(33, None if y is None else cuda(y, dtype)[:33])
    assert zz.shape == (33,) + tuple(shape) and ll.shape == (33,) and zz.dtype == dtype and torch.isfinite(ll).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("temperature", [None, 0.7])
@pytest.mark.parametrize("labels", ["hard", "soft", "none"])
@pytest.mark.parametrize("shape", GLOW_SHAPES, ids=str)
def test_glow_base_log_prob_and_from_noise(hip, shape, labels, temperature, dtype):
    _density_and_sampling("glow", shape, labels, temperature, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("temperature", [None, 0.7])
@pytest.mark.parametrize("labels", ["hard", "soft"])
@pytest.mark.parametrize("shape", CCDG_SHAPES, ids=str)
def test_class_cond_diag_gaussian_log_prob_and_from_noise(hip, shape, labels, temperature, dtype):
    _density_and_sampling("ccdg", shape, labels, temperature, dtype)


# ---------------------------------------------------------------- gradients
def _ref_grads(kind, shape, direction, temperature, params, y, x, w, gz, dtype):
    """Torch autograd on the restatement: d loss / d (input, every parameter, a float y)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    p = {k: leaf(v) for k, v in params.items()}
    x = leaf(x)
    y = leaf(y) if (y is not None and y.is_floating_point()) else y
    tables = KINDS[kind][1](p, y, shape)
    if direction == "log_prob":
        loss = (ref_log_prob(x, *tables, temperature) * w.to(dtype)).sum()
    else:
        z, lp = ref_sample(x, *tables, temperature)
        loss = (lp * w.to(dtype)).sum() + (z * gz.to(dtype)).sum()
    loss.backward()
    out = {"input": x.grad}
    out.update({k: v.grad for k, v in p.items()})
    if y is not None and y.is_floating_point():
        out["y"] = y.grad
    assert all(torch.isfinite(v).all() for v in out.values())
    return out


def _hip_grads(q, direction, y, x, w, gz):
    q.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_()
    y = y.clone().requires_grad_() if (y is not None and y.is_floating_point()) else y
    if direction == "log_prob":
        loss = (q.log_prob(x, y) * w).sum()
    else:
        z, lp = q.from_noise(x, y)
        loss = (lp * w).sum() + (z * gz).sum()
    loss.backward()
    out = {"input": x.grad}
    out.update({k: v.grad for k, v in q.named_parameters()})
    if y is not None and y.is_floating_point():
        out["y"] = y.grad
    return {k: v.clone() for k, v in out.items()}


GRAD_CASES = [("glow", (12, 8, 8), "hard"), ("glow", (12, 8, 8), "soft"), ("glow", (5, 3, 3), "hard"),
              ("glow", (7,), "soft"), ("glow", (6, 16, 16), "none"), ("glow", (48, 4, 4), "hard"),
              ("ccdg", (64,), "hard"), ("ccdg", (64,), "soft"), ("ccdg", (6, 4, 4), "hard"), ("ccdg", (1000,), "soft")]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("direction", ["log_prob", "sample"])
@pytest.mark.parametrize("kind,shape,labels", GRAD_CASES, ids=lambda v: str(v))
def test_gradients_match_autograd_on_the_restatement(hip, kind, shape, labels, direction, dtype):
    """Loss sum(log_prob w), or sum(logp w) + sum(z gz) for sampling, with random w and gz; gradients with respect to
    the input, every parameter and a float y.  fp32: helpers.parity against the restatement's fp32 and fp64 autograd.
    fp64: rtol 1e-9; a parameter gradient is a sum of up to B * P ~ 1e6 terms that cancel, so its rounding error scales
    with the size of the terms rather than of the result: the absolute tolerance is 1e-9 x the largest entry of that
    gradient tensor (at least 1e-9).  Two backward passes give the same bits."""
    g = torch.Generator().manual_seed(seed_of(kind, shape, labels, direction))
    nc = None if labels == "none" else NC
    temperature = 0.7 if direction == "sample" else None
    params = {k: v.to(dtype) for k, v in draw_params(kind, shape, nc, g).items()}
    y = cast(draw_labels(labels, g), dtype)
    x = torch.randn(B, *shape, generator=g, dtype=torch.float64).to(dtype)
    w = torch.randn(B, generator=g, dtype=torch.float64).to(dtype)
    gz = torch.randn(B, *shape, generator=g, dtype=torch.float64).to(dtype)
    r64 = _ref_grads(kind, shape, direction, temperature, params, y, x, w, gz, torch.float64)
    r32 = _ref_grads(kind, shape, direction, temperature, params, y, x, w, gz, torch.float32) if dtype == torch.float32 else None
    q = build(kind, shape, nc, params, dtype)
    q.temperature = temperature
    args = (q, direction, None if y is None else y.cuda(), x.cuda(), w.cuda(), gz.cuda())
    got = _hip_grads(*args)
    again = _hip_grads(*args)
    assert sorted(got) == sorted(r64)
    for k in sorted(got):
        assert got[k] is not None and got[k].dtype == dtype, k
        assert torch.equal(got[k], again[k]), "gradient of %s differs between two backward passes" % k
        if dtype == torch.float32:
            parity(got[k], r32[k], r64[k], what="d/d" + k)
        else:
            assert_close(got[k], r64[k], rtol=1e-9, atol=1e-9 * max(1.0, float(r64[k].abs().max())), what="d/d" + k)


# ---------------------------------------------------------------- labels outside the table
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind,shape", [("glow", (12, 8, 8)), ("glow", (5, 3, 3)), ("ccdg", (64,)), ("ccdg", (6, 3, 3))], ids=str)
def test_out_of_range_labels_give_nan_for_those_samples_only(hip, kind, shape, dtype):
    """A label equal to num_classes and a label of -1: the kernel's guard reads nothing outside the table and writes
    NaN for exactly those samples; every other sample has the bits of the run with valid labels."""
    g = torch.Generator().manual_seed(29)
    params = draw_params(kind, shape, NC, g)
    y = draw_labels("hard", g)
    x = torch.randn(B, *shape, generator=g, dtype=torch.float64).to(dtype).cuda()
    q = build(kind, shape, NC, params, dtype)
    bad = torch.zeros(B, dtype=torch.bool)
    y_bad = y.clone()
    y_bad[5], y_bad[B - 3] = NC, -1
    bad[5] = bad[B - 3] = True
    bad = bad.cuda()
    rows = lambda t: torch.isnan(t.reshape(B, -1)).all(1)
    some = lambda t: torch.isnan(t.reshape(B, -1)).any(1)
    with torch.no_grad():
        lp, lp_bad = q.log_prob(x, y.cuda()), q.log_prob(x, y_bad.cuda())
        (z, lq), (z_bad, lq_bad) = q.from_noise(x, y.cuda()), q.from_noise(x, y_bad.cuda())
    for clean, dirty in ((lp, lp_bad), (lq, lq_bad), (z, z_bad)):
        assert not torch.isnan(clean).any()
        assert torch.equal(rows(dirty), bad) and torch.equal(some(dirty), bad)
        assert torch.equal(dirty[~bad], clean[~bad])
    # the VJP: NaN input-gradient rows for those samples, the parameter gradients take the other samples only
    xg = x.clone().requires_grad_()
    (torch.nan_to_num(q.log_prob(xg, y_bad.cuda())) * 1.0).sum().backward()
    assert torch.equal(rows(xg.grad), bad) and torch.equal(some(xg.grad), bad)
    assert all(torch.isfinite(p.grad).all() for p in q.parameters())


# ---------------------------------------------------------------- ClassCondFlow
def _cc_flow_parts(dtype, seed=41):
    torch.manual_seed(seed)
    flows = []
    for _ in range(4):
        flows += [nf.flows.AffineCouplingBlock(nf.nets.MLP([4, 16, 16, 8], init_zeros=False)), nf.flows.Permute(8, mode="swap")]
    g = torch.Generator().manual_seed(seed)
    params = draw_params("ccdg", (8,), NC, g)
    q0 = nf.distributions.ClassCondDiagGaussian(8, NC)
    q0.load_state_dict({k: v.float() for k, v in params.items()})
    model = nf.ClassCondFlow(q0, flows).to(dtype).cuda()
    return model, {k: v.float().to(dtype) for k, v in params.items()}, g


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_class_cond_flow_log_prob_sample_and_training(hip, dtype):
    """[AffineCouplingBlock(MLP), Permute] x 4 + ClassCondDiagGaussian(8, 10).  log_prob(x, y) against the same flow
    modules walked by an existing NormalizingFlow plus the restated base on the latent that walk ends in; sample_from
    then log_prob reproduces log q to 1e-4 (1 + |log q|) in fp32 - the round-trip figure of the affine stacks in
    test_gpu_parity.py: the latent comes back to a few fp32 roundings per coupling, and the base's quadratic term
    amplifies that by |u| <= ~5 - and to 1e-10 in fp64; forward_kld(x, y).backward() reaches every parameter."""
    model, params, g = _cc_flow_parts(dtype)
    model.eval()
    y = draw_labels("hard", g)
    x = torch.randn(B, 8, generator=g, dtype=torch.float64).to(dtype)
    plain = nf.NormalizingFlow(nf.distributions.DiagGaussian(8), list(model.flows)).to(dtype).cuda().eval()
    with torch.no_grad():
        lp = model.log_prob(x.cuda(), y.cuda())
        z, log_det = plain._walk(x.cuda(), torch.zeros(B, dtype=dtype, device="cuda"), None, True)
    z, log_det = z.cpu(), log_det.cpu()
    want = {dt: log_det.to(dt) + ref_log_prob(z.to(dt), *ccdg_tables({k: v.to(dt) for k, v in params.items()}, y, (8,)), None)
            for dt in (torch.float32, torch.float64)}
    assert all(torch.isfinite(v).all() for v in want.values())
    check(lp, want[torch.float32], want[torch.float64], dtype, "ClassCondFlow.log_prob")
    eps = torch.randn(B, 8, generator=g, dtype=torch.float64).to(dtype).cuda()
    with torch.no_grad():
        zs, lq = model.sample_from(eps, y.cuda())
        back = model.log_prob(zs, y.cuda())
        z1, l1 = model.sample(16, y.cuda()[:16])
        z2, l2 = model.sample(9)
    tol = 1e-4 if dtype == torch.float32 else 1e-10
    assert torch.isfinite(lq).all()
    assert float(((back - lq).abs() / (1.0 + lq.abs())).max()) <= tol
    assert z1.shape == (16, 8) and l1.shape == (16,) and z2.shape == (9, 8) and torch.isfinite(l2).all()
    model.train()
    loss = model.forward_kld(x.cuda(), y.cuda())
    loss.backward()
    assert torch.isfinite(loss)
    assert_close(loss, -want[torch.float64].mean(), rtol=1e-5 if dtype == torch.float32 else 1e-10, atol=1e-5, what="forward_kld")
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert float(model.q0.loc.grad.abs().sum()) > 0 and float(model.q0.log_scale.grad.abs().sum()) > 0


def test_class_cond_flow_save_load(hip, tmp_path):
    model, _, g = _cc_flow_parts(torch.float32)
    twin, _, _ = _cc_flow_parts(torch.float32, seed=43)
    path = str(tmp_path / "ccflow.pt")
    model.save(path)
    twin.load(path)
    x, y = torch.randn(64, 8, generator=g).cuda(), torch.randint(NC, (64,), generator=g).cuda()
    with torch.no_grad():
        assert torch.equal(model.eval().log_prob(x, y), twin.eval().log_prob(x, y))


# ---------------------------------------------------------------- MultiscaleFlow(class_cond=True)
def _glow_pair(base_params=None, seed=1101):
    """A tiny 2-level Glow (fixture G11's architecture and synthetic weights) twice over the SAME flow modules: with
    GlowBase(num_classes=10) bases and class_cond=True, and with standard-normal DiagGaussian bases and
    class_cond=False (the existing, fixture-tested path)."""
    levels, blocks, hidden, inp = 2, 2, 16, (3, 8, 8)
    merges, flows, shapes = [], [], []
    for i in range(levels):
        fl = [nf.flows.GlowBlock(inp[0] * 2 ** (levels + 1 - i), hidden, split_mode="channel", scale=True) for _ in range(blocks)]
        flows += [fl + [nf.flows.Squeeze()]]
        if i > 0:
            merges += [nf.flows.Merge()]
            shapes += [(inp[0] * 2 ** (levels - i), inp[1] // 2 ** (levels - i), inp[2] // 2 ** (levels - i))]
        else:
            shapes += [(inp[0] * 2 ** (levels + 1), inp[1] // 2 ** levels, inp[2] // 2 ** levels)]
    plain = nf.MultiscaleFlow([nf.distributions.DiagGaussian(s) for s in shapes], flows, merges, class_cond=False)
    sd = glow_state(fixture("g11_glow_multiscale"), seed)
    plain.load_state_dict({k: (torch.zeros_like(v) if k.startswith("q0.") else v) for k, v in sd.items()})
    cc = nf.MultiscaleFlow([nf.distributions.GlowBase(s, NC) for s in shapes], flows, merges, class_cond=True)
    if base_params is not None:
        for q, p in zip(cc.q0, base_params):
            q.load_state_dict({k: v.float() for k, v in p.items()})
    return cc.cuda().eval(), plain.cuda().eval(), shapes


def _record_latents(model):
    """Make every base of ``model`` note the latent it is asked to score."""
    seen = {}
    for i, q in enumerate(model.q0):
        def log_prob(z, *a, _i=i, _q=q, **k):
            seen[_i] = z.detach().cpu()
            return type(_q).log_prob(_q, z, *a, **k)
        q.log_prob = log_prob
    return seen


def _glow_inputs(n, seed=77):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(NC, (n,), generator=g)
    return torch.rand(n, 3, 8, 8, generator=g), y, g


def test_multiscale_zero_bases_equal_the_plain_path(hip):
    """(a) All base parameters zero: GlowBase is the standard normal, so log_prob(x, y) is the DiagGaussian /
    class_cond=False model's log_prob (parity with both references taken as that path)."""
    cc, plain, _ = _glow_pair()
    x, y, _ = _glow_inputs(256)
    with torch.no_grad():
        got, want = cc.log_prob(x.cuda(), y.cuda()), plain.log_prob(x.cuda()).cpu()
    assert torch.isfinite(want).all() and len(torch.unique(y)) == NC
    parity(got, want, want.double(), what="zero class-conditional bases")


def test_multiscale_random_bases_shift_log_prob_by_the_restated_base_terms(hip):
    """(b) Random base parameters: log_prob(x, y) - log_prob_plain(x) is the sum over levels of the restated GlowBase
    log-density minus the standard-normal log-density, on the latents each level's base is given."""
    g = torch.Generator().manual_seed(5)
    shapes = [(24, 2, 2), (6, 4, 4)]
    base_params = [draw_params("glow", s, NC, g) for s in shapes]
    cc, plain, got_shapes = _glow_pair(base_params)
    assert got_shapes == shapes
    x, y, _ = _glow_inputs(256)
    seen = _record_latents(plain)
    with torch.no_grad():
        got = cc.log_prob(x.cuda(), y.cuda())
        lp_plain = plain.log_prob(x.cuda()).cpu()
    assert sorted(seen) == [0, 1]
    want = {}
    for dt in (torch.float32, torch.float64):
        total = lp_plain.to(dt)
        for i, s in enumerate(shapes):
            z = seen[i].to(dt)
            p = {k: v.float().to(dt) for k, v in base_params[i].items()}
            std = -0.5 * z[0].numel() * math.log(2 * math.pi) - 0.5 * (z ** 2).sum(dim=[1, 2, 3])
            total = total + ref_log_prob(z, *glow_tables(p, y, s), None) - std
        want[dt] = total
    assert all(torch.isfinite(v).all() for v in want.values()) and len(torch.unique(y)) == NC
    assert float((want[torch.float64] - lp_plain.double()).abs().min()) > 1e-3        # the bases really moved it
    parity(got, want[torch.float32], want[torch.float64], what="class-conditional multiscale log_prob")


def test_multiscale_sampling_with_labels_and_temperature(hip):
    """(c) sample(num_samples, y, temperature=0.7): shapes, temperature restored; sample_from(noise, y) then
    log_prob(., y) reproduces log q to 1e-4 (1 + |log q|), the fp32 round-trip figure used for ClassCondFlow above
    (more couplings here, inputs of a few hundred elements: log q ~ 1e2-1e3, so this is ~1e-1 absolute at most)."""
    g = torch.Generator().manual_seed(6)
    shapes = [(24, 2, 2), (6, 4, 4)]
    cc, _, _ = _glow_pair([draw_params("glow", s, NC, g) for s in shapes])
    _, y, _ = _glow_inputs(64)
    with torch.no_grad():
        z, lq = cc.sample(64, y.cuda(), temperature=0.7)
        assert z.shape == (64, 3, 8, 8) and lq.shape == (64,) and torch.isfinite(lq).all()
        assert all(q.temperature is None for q in cc.q0)
        z, lq = cc.sample(5)
        assert z.shape == (5, 3, 8, 8) and lq.shape == (5,)
        noise = [torch.randn(64, *s, generator=g).cuda() for s in shapes]
        z, lq = cc.sample_from(noise, y.cuda())
        back = cc.log_prob(z, y.cuda())
        other = cc.log_prob(z, ((y + 1) % NC).cuda())
    assert torch.isfinite(z).all()
    assert float(((back - lq).abs() / (1.0 + lq.abs())).max()) <= 1e-4
    assert float((other - lq).abs().min()) > 1e-2             # the labels matter


def test_multiscale_class_conditional_training(hip):
    """(d) Twenty Adam steps of forward_kld(x, y) in fp32 on a fixed batch whose classes have different means: the loss
    after them is strictly lower than at the start and loc_cc received a non-zero gradient on the first step."""
    cc, _, _ = _glow_pair()
    cc.train()
    x, y, g = _glow_inputs(256, seed=88)
    x = (0.25 * x + 0.07 * y.view(-1, 1, 1, 1).float()).cuda()
    y = y.cuda()
    opt = torch.optim.Adam(cc.parameters(), lr=1e-3)
    losses = []
    for step in range(20):
        opt.zero_grad()
        loss = cc.forward_kld(x, y)
        loss.backward()
        if step == 0:
            assert all(float(q.loc_cc.grad.abs().sum()) > 0 for q in cc.q0)
            assert all(p.grad is None or torch.isfinite(p.grad).all() for p in cc.parameters())
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float(cc.forward_kld(x, y))
    print("class-conditional Glow forward_kld: %.4f -> %.4f" % (losses[0], final))
    assert np.isfinite(losses).all() and final < losses[0], losses


# ---------------------------------------------------------------- graph capture
def test_class_cond_flow_log_prob_is_capturable(hip):
    """ClassCondFlow.log_prob(x_static, y_static) under torch.cuda.graph (one stream, side-stream warm-up as
    vcnf_amd.graphs does): new inputs and labels copied into the static buffers, replay equals the eager result."""
    model, _, g = _cc_flow_parts(torch.float32)
    model.eval()
    n = 512
    draw = lambda: (torch.randn(n, 8, generator=g).cuda(), torch.randint(NC, (n,), generator=g).cuda())
    x_static, y_static = draw()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            model.log_prob(x_static, y_static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = model.log_prob(x_static, y_static)
    for _ in range(2):
        x, y = draw()
        x_static.copy_(x)
        y_static.copy_(y)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = model.log_prob(x, y)
        assert torch.isfinite(eager).all() and torch.equal(out, eager)
