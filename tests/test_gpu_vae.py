"""The flow VAE's end caps on the HIP kernels (csrc/vae_ends.hip) and NormalizingFlowVAE on the device.

The reference is the plain-torch restatement in vae_ref.py, run on the CPU in fp32 and in fp64 on the inputs as the
kernels see them.  fp32 results are judged by helpers.parity (against the restatement's fp32 run, with its own
fp32-vs-fp64 error as the yardstick); fp64 results by rtol = atol = 1e-10.  Before anything is compared the
restatement's outputs are checked to be finite in both precisions.  Inputs are seeded (vae_ref.inputs); gradients are
those of sum_k <output_k, cotangent_k> with seeded standard-normal cotangents, against torch.autograd.grad of the
restatement."""
import pytest
import torch
from torch import nn

import vae_ref as ref
import vcnf_amd as nf
from helpers import assert_close, parity
from vcnf_amd import _lib, vae_ends

pytestmark = pytest.mark.gpu

# (feature shape, B, S).  D = 1, 2, 7: partial lane groups; 64: sixteen (fp64: thirty-two) chunks; 257: a scalar row
# longer than a group's first trip with a ragged last chunk; 784: 16-byte packs with a pack-aligned lv half; 6: 8-byte
# packs in fp32 with a half chunk at the end; batches that leave the last workgroup partial, S = 1 (the loop-free VJP),
# and an image shape
CASES = [(d, 5, 3) for d in (1, 2, 6, 7, 64, 257, 784)] + [(7, 1, 1), (7, 63, 1), (7, 64, 4), ((2, 3, 3), 5, 3)]
F64 = dict(rtol=1e-10, atol=1e-10)
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
KERNELS = ("encode", "encode_bwd", "gauss_log_prob", "gauss_log_prob_bwd", "bernoulli_log_prob", "bernoulli_log_prob_bwd")
cast = ref.cast


def case_id(case):
    return "%s-B%d-S%d" % (str(case[0]).replace(" ", ""), case[1], case[2])


def as_tuple(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def references(fn, dtype, *tensors):
    """fn on the CPU: (fp32 run or None, fp64 run) of the inputs rounded to ``dtype``, as tuples; every output finite."""
    seen = [cast(t, dtype) for t in tensors]
    r64 = as_tuple(fn(*[cast(t, torch.float64) for t in seen]))
    r32 = as_tuple(fn(*[cast(t, torch.float32) for t in seen])) if dtype == torch.float32 else None
    for r in (r64, r32):
        for t in (r or ()):
            assert torch.isfinite(t).all(), "the reference output is not finite"
    return r32, r64


def check(got, r32, r64, dtype, what):
    assert got.dtype == dtype, what
    got = got.detach().reshape(r64.shape)
    print("%s %s max |got - fp64 reference| %.3e of %.3e" % (what, dtype, float((got.cpu().double() - r64).abs().max()),
                                                            float(r64.abs().max())))
    if dtype == torch.float32:
        parity(got, r32, r64, what=what)
    else:
        assert_close(got, r64, what=what, **F64)


def check_all(got, r32, r64, dtype, what):
    got = as_tuple(got)
    assert len(got) == len(r64)
    for i, g in enumerate(got):
        check(g, r32 and r32[i], r64[i], dtype, "%s[%d]" % (what, i))


def cuda(t, dtype):
    return cast(t, dtype).cuda()


def vjp(fn, wrt, n_in):
    """The function (inputs..., cotangents...) -> gradients of sum_k <fn(inputs)[k], cotangent_k> with respect to the
    inputs ``wrt``; a cotangent that is None leaves its output out."""
    def run(*tensors):
        ins = [t.detach().clone().requires_grad_(i in wrt) for i, t in enumerate(tensors[:n_in])]
        outs = as_tuple(fn(*ins))
        loss = sum((o * c.reshape(o.shape)).sum() for o, c in zip(outs, tensors[n_in:]) if c is not None)
        return torch.autograd.grad(loss, [ins[i] for i in wrt])
    return run


def cotangent(shape, *key):
    g = torch.Generator().manual_seed(ref.seed_of("cotangent", shape, *key))
    return torch.randn(shape, generator=g, dtype=torch.float64)


def count_calls(monkeypatch):
    """Names of the _lib.vae_* wrappers in the order they are called from here on."""
    calls = []
    for k in KERNELS:
        fn = getattr(_lib, "vae_" + k)
        monkeypatch.setattr(_lib, "vae_" + k, lambda *a, _fn=fn, _k=k, **kw: calls.append(_k) or _fn(*a, **kw))
    return calls


def compare(ref_fn, hip_fn, dtype, tensors, what, wrt=None, n_in=None, twice=True):
    """ref_fn on the CPU against hip_fn on the device on the same tensors (the forward, or with ``wrt`` its VJP)."""
    if wrt is not None:
        ref_fn, hip_fn = vjp(ref_fn, wrt, n_in), vjp(hip_fn, wrt, n_in)
    r32, r64 = references(ref_fn, dtype, *tensors)
    on_device = [None if t is None else cuda(t, dtype) for t in tensors]
    with torch.set_grad_enabled(wrt is not None):
        got = as_tuple(hip_fn(*on_device))
        again = as_tuple(hip_fn(*on_device)) if twice else got
    check_all(got, r32, r64, dtype, what)
    for a, b in zip(got, again):
        assert torch.equal(a, b), what + ": the same call twice gives different bits"
    return got


# ---------------------------------------------------------------- 1. the encoder's draw
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_encode(hip, case, dtype, monkeypatch):
    shape, b, s = case
    t = ref.inputs("encode", b, s, shape)
    calls = count_calls(monkeypatch)
    z, lq = compare(ref.encode, _lib.vae_encode, dtype, (t["h"], t["eps"]), "encode")
    assert z.shape == t["eps"].shape and lq.shape == (b, s)
    assert calls == ["encode"] * 2
    del calls[:]
    g_z, g_lq = cotangent(tuple(t["eps"].shape), "z"), cotangent((b, s), "lq")
    for cots, what in (((g_z, g_lq), "both"), ((None, g_lq), "g_z absent"), ((g_z, None), "g_lq absent")):
        d_h, = compare(ref.encode, vae_ends.encode, dtype, (t["h"], t["eps"]) + cots, "encode VJP, " + what, wrt=(0,), n_in=2)
        assert d_h.shape == t["h"].shape
    assert calls == ["encode", "encode_bwd"] * 6


# ---------------------------------------------------------------- 2. the Gaussian log-likelihood, both roles
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("role", ["gauss_z", "gauss_x"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gauss_log_prob(hip, case, role, dtype, monkeypatch):
    shape, b, s = case
    t = ref.inputs(role, b, s, shape)
    divs = (1, s) if role == "gauss_z" else (s, 1)
    fn = lambda f: (lambda v, h: f(v, h, *divs))
    calls = count_calls(monkeypatch)
    lp, = compare(fn(ref.gauss_log_prob), fn(_lib.vae_gauss_log_prob), dtype, (t["v"], t["h"]), role)
    assert lp.shape == (b * s,)
    g = cotangent((b * s,), role)
    both = compare(fn(ref.gauss_log_prob), fn(vae_ends.gauss_log_prob), dtype, (t["v"], t["h"], g), role + " VJP", wrt=(0, 1), n_in=2)
    d_v, = compare(fn(ref.gauss_log_prob), fn(vae_ends.gauss_log_prob), dtype, (t["v"], t["h"], g), role + " VJP, d_v only", wrt=(0,), n_in=2)
    d_h, = compare(fn(ref.gauss_log_prob), fn(vae_ends.gauss_log_prob), dtype, (t["v"], t["h"], g), role + " VJP, d_h only", wrt=(1,), n_in=2)
    assert torch.equal(d_v, both[0]) and torch.equal(d_h, both[1])
    assert d_v.shape == t["v"].shape and d_h.shape == t["h"].shape
    assert calls == ["gauss_log_prob"] * 2 + ["gauss_log_prob", "gauss_log_prob_bwd"] * 6


# ---------------------------------------------------------------- 3. the Bernoulli log-likelihood
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_bernoulli_log_prob(hip, case, dtype, monkeypatch):
    shape, b, s = case
    t = ref.inputs("bernoulli", b, s, shape)
    fn = lambda f: (lambda x, a: f(x, a, s))
    calls = count_calls(monkeypatch)
    lp, = compare(fn(ref.bernoulli_log_prob), fn(_lib.vae_bernoulli_log_prob), dtype, (t["x"], t["score"]), "bernoulli")
    assert lp.shape == (b * s,)
    g = cotangent((b * s,), "bernoulli")
    d_a, = compare(fn(ref.bernoulli_log_prob), fn(vae_ends.bernoulli_log_prob), dtype, (t["x"], t["score"], g), "bernoulli VJP",
                   wrt=(1,), n_in=2)
    assert d_a.shape == t["score"].shape
    assert calls == ["bernoulli_log_prob"] * 2 + ["bernoulli_log_prob", "bernoulli_log_prob_bwd"] * 2


# ---------------------------------------------------------------- 4. stiff inputs
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stiff_encoder(hip, dtype):
    """lv = +100 on item 0 and -100 on item 1: standard deviations e^50 and e^-50."""
    b, s, d = 5, 3, 7
    t = ref.inputs("encode", b, s, d)
    t["h"][0, d:], t["h"][1, d:] = 100.0, -100.0
    got = compare(ref.encode, _lib.vae_encode, dtype, (t["h"], t["eps"]), "stiff encode")
    cots = (cotangent((b, s, d), "stiff z"), cotangent((b, s), "stiff lq"))
    got += compare(ref.encode, vae_ends.encode, dtype, (t["h"], t["eps"]) + cots, "stiff encode VJP", wrt=(0,), n_in=2)
    assert all(torch.isfinite(g).all() for g in got)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("role", ["gauss_z", "gauss_x"])
def test_stiff_gauss_log_prob(hip, role, dtype):
    """lv = +10 and -10 on the first two parameter rows."""
    b, s, d = 5, 3, 7
    t = ref.inputs(role, b, s, d)
    t["h"][0, d:], t["h"][1, d:] = 10.0, -10.0
    divs = (1, s) if role == "gauss_z" else (s, 1)
    fn = lambda f: (lambda v, h: f(v, h, *divs))
    got = compare(fn(ref.gauss_log_prob), fn(_lib.vae_gauss_log_prob), dtype, (t["v"], t["h"]), "stiff " + role)
    got += compare(fn(ref.gauss_log_prob), fn(vae_ends.gauss_log_prob), dtype, (t["v"], t["h"], cotangent((b * s,), "stiff", role)),
                   "stiff %s VJP" % role, wrt=(0, 1), n_in=2)
    assert all(torch.isfinite(g).all() for g in got)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stiff_bernoulli(hip, dtype):
    """Scores +-80 and +-1e4 against x = 0, 1 and 0.3."""
    b, s, d = 5, 3, 7
    t = ref.inputs("bernoulli", b, s, d)
    t["x"][2] = 0.3
    for item in range(3):                                    # x = 0, 1, 0.3
        for k in range(s):
            t["score"][item * s + k, :4] = torch.tensor([80.0, -80.0, 1e4, -1e4], dtype=torch.float64)
    fn = lambda f: (lambda x, a: f(x, a, s))
    got = compare(fn(ref.bernoulli_log_prob), fn(_lib.vae_bernoulli_log_prob), dtype, (t["x"], t["score"]), "stiff bernoulli")
    got += compare(fn(ref.bernoulli_log_prob), fn(vae_ends.bernoulli_log_prob), dtype, (t["x"], t["score"], cotangent((b * s,), "stiff b")),
                   "stiff bernoulli VJP", wrt=(1,), n_in=2)
    assert all(torch.isfinite(g).all() for g in got)


# ---------------------------------------------------------------- 5. alignment
def offset_by_one(t):
    """The same values in a view that starts at element 1 of a larger buffer."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() == buf.data_ptr() + t.element_size() and view.is_contiguous()
    return view


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("d", [6, 784])
def test_an_offset_base_pointer_changes_no_bit(hip, d, dtype):
    """16-byte (D = 784) and 8-byte (D = 6 in fp32) accesses against the scalar accesses an offset base forces."""
    b, s = 5, 3
    enc, gz, gx, ber = ({n: cuda(v, dtype) for n, v in ref.inputs(k, b, s, d).items()} for k in ref.KINDS)
    assert all(v.data_ptr() % 16 == 0 for t in (enc, gz, gx, ber) for v in t.values())
    off = offset_by_one
    with torch.no_grad():
        for which in ((True, True), (True, False), (False, True)):      # each operand on its own and both
            sh = lambda a, i: off(a) if which[i] else a
            for got, want in zip(_lib.vae_encode(sh(enc["h"], 0), sh(enc["eps"], 1)), _lib.vae_encode(enc["h"], enc["eps"])):
                assert torch.equal(got, want), "encode %s" % (which,)
            assert torch.equal(_lib.vae_gauss_log_prob(sh(gz["v"], 0), sh(gz["h"], 1), 1, s), _lib.vae_gauss_log_prob(gz["v"], gz["h"], 1, s))
            assert torch.equal(_lib.vae_gauss_log_prob(sh(gx["v"], 0), sh(gx["h"], 1), s, 1), _lib.vae_gauss_log_prob(gx["v"], gx["h"], s, 1))
            assert torch.equal(_lib.vae_bernoulli_log_prob(sh(ber["x"], 0), sh(ber["score"], 1), s),
                               _lib.vae_bernoulli_log_prob(ber["x"], ber["score"], s))


# ---------------------------------------------------------------- 6. the sample limit
def _limit_case(kind, s):
    """(restatement, device function, tensors, wrt, rows) of the VJP at B = 1, D = 2 with S samples.  ``rows``: None, or
    (position in wrt of the gradient that is a sum over the S rows, the function and tensors that give the S terms of
    that sum one per row: the same arithmetic at B = S, one sample each, with the shared operand repeated)."""
    t = ref.inputs(kind, 1, s, 2)
    if kind == "encode":
        g_z, g_lq = cotangent((1, s, 2), "limit z"), cotangent((1, s), "limit lq")
        rows = (0, vjp(ref.encode, (0,), 2), (ref.repeat_rows(t["h"], s), t["eps"].reshape(s, 1, 2), g_z.reshape(s, 1, 2), g_lq.reshape(s, 1)))
        return ref.encode, vae_ends.encode, (t["h"], t["eps"], g_z, g_lq), (0,), rows
    if kind == "bernoulli":
        fn = lambda f: (lambda x, a: f(x, a, s))
        return fn(ref.bernoulli_log_prob), fn(vae_ends.bernoulli_log_prob), (t["x"], t["score"], cotangent((s,), "limit b")), (1,), None
    g = cotangent((s,), "limit", kind)
    divs = (1, s) if kind == "gauss_z" else (s, 1)
    fn = lambda f: (lambda v, h: f(v, h, *divs))
    if kind == "gauss_z":
        rows = (1, vjp(ref.gauss_log_prob, (1,), 2), (t["v"], ref.repeat_rows(t["h"], s), g))
    else:
        rows = (0, vjp(ref.gauss_log_prob, (0,), 2), (ref.repeat_rows(t["v"], s), t["h"], g))
    return fn(ref.gauss_log_prob), fn(vae_ends.gauss_log_prob), (t["v"], t["h"], g), (0, 1), rows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_sample_limit(hip, kind, dtype, monkeypatch):
    """B = 1, D = 2: S = 4096 is the VJP kernel's longest walk; S = 4097 makes no kernel call and gives the composition's
    gradients.  Without autograd the forward kernel takes S = 4097.

    At S = 4096 the shared operand's gradient is a sum of 4096 terms that the kernel adds one after the other, which in
    fp32 is less accurate than the restatement's pairwise torch.sum: helpers.parity, whose yardstick is the restatement's
    own fp32 error, does not apply to it.  It is judged against the fp64 restatement by the bound of sequential
    summation, |error| <= (S - 1) 2^-24 sum_s |term_s| (terms from the restatement, one row each), on top of the 2e-5
    elementwise tolerance of parity for the terms themselves.  fp64, and every per-row output, is judged as elsewhere."""
    s = 4096
    assert _lib.VAE_MAX_SAMPLES == s
    calls = count_calls(monkeypatch)
    ref_fn, hip_fn, tensors, wrt, rows = _limit_case(kind, s)
    r32, r64 = references(vjp(ref_fn, wrt, 2), dtype, *tensors)
    got = vjp(hip_fn, wrt, 2)(*[cuda(t, dtype) for t in tensors])
    assert len(calls) == 2 and calls[1].endswith("_bwd"), calls
    for i in range(len(wrt)):
        if dtype == torch.float32 and rows is not None and i == rows[0]:
            terms, = references(rows[1], torch.float64, *[cast(t, dtype) for t in rows[2]])[1]
            assert_close(terms.sum(0, keepdim=True), r64[i], what="the rows' terms add up to the gradient", **F64)
            bound = (s - 1) * 2.0 ** -24 * terms.abs().sum(0, keepdim=True)
            err = (got[i].cpu().double() - r64[i]).abs()
            print("%s summed gradient: max error %.3e, bound there %.3e" % (kind, float(err.max()), float(bound.reshape(-1)[err.argmax()])))
            assert got[i].dtype == dtype and bool((err <= bound + 2e-5 + 2e-5 * r64[i].abs()).all()), kind
        else:
            check(got[i], r32 and r32[i], r64[i], dtype, "%s at the limit [%d]" % (kind, i))
    del calls[:]
    ref_fn, hip_fn, tensors, wrt, _ = _limit_case(kind, s + 1)
    compare(ref_fn, hip_fn, dtype, tensors, "%s over the limit" % kind, wrt=wrt, n_in=2, twice=False)
    assert calls == []
    compare(ref_fn, hip_fn, dtype, tensors[:2], "%s forward over the limit" % kind, twice=False)
    assert len(calls) == 1 and not calls[0].endswith("_bwd")


# ---------------------------------------------------------------- 7. which path runs
def _ends(dtype, fuse=True):
    torch.manual_seed(21)
    D = nf.distributions
    mods = (D.NNDiagGaussian(nn.Linear(6, 8), fuse=fuse), D.NNBernoulliDecoder(nn.Linear(4, 6), fuse=fuse),
            D.NNDiagGaussianDecoder(nn.Linear(4, 12), fuse=fuse))
    x = torch.rand(5, 6, generator=torch.Generator().manual_seed(22), dtype=torch.float64)
    return [m.to(dtype).cuda() for m in mods], x.to(dtype).cuda()


def _run_ends(mods, x, s=3):
    enc, ber, gau = mods
    z, lq = enc(x, num_samples=s)
    lq2 = enc.log_prob(z, x)
    flat = z.reshape(-1, 4)
    return z, lq, lq2, ber.log_prob(x, flat), gau.log_prob(x, flat)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kernel_path_is_one_call_per_end_cap(hip, dtype, monkeypatch):
    calls = count_calls(monkeypatch)
    mods, x = _ends(dtype)
    with torch.no_grad():
        torch.manual_seed(1)
        fused = _run_ends(mods, x)
    assert calls == ["encode", "gauss_log_prob", "bernoulli_log_prob", "gauss_log_prob"]
    del calls[:]
    plain_mods, _ = _ends(dtype, fuse=False)
    with torch.no_grad():
        torch.manual_seed(1)
        plain = _run_ends(plain_mods, x)
    assert calls == []
    tol = dict(rtol=2e-5, atol=2e-5) if dtype == torch.float32 else F64
    for a, b_, what in zip(fused, plain, ("z", "log_q", "log_prob(z, x)", "bernoulli", "gaussian decoder")):
        assert a.shape == b_.shape and a.dtype == dtype
        assert_close(a, b_, what="fuse=True against fuse=False: " + what, **tol)
    assert_close(fused[1], fused[2], what="log_prob of the draw", **tol)
    # with autograd recording: one forward and one backward call per end cap
    torch.manual_seed(1)
    out = _run_ends(mods, x)
    assert calls == ["encode", "gauss_log_prob", "bernoulli_log_prob", "gauss_log_prob"]
    del calls[:]
    sum(o.sum() for o in out[1:]).backward()
    assert sorted(calls) == sorted(["encode_bwd", "gauss_log_prob_bwd", "bernoulli_log_prob_bwd", "gauss_log_prob_bwd"])
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for m in mods for p in m.parameters())


def test_half_precision_and_data_gradients_take_the_composition(hip, monkeypatch):
    calls = count_calls(monkeypatch)
    mods, x = _ends(torch.float16)
    out = _run_ends(mods, x)
    assert calls == [] and all(o.dtype == torch.float16 and torch.isfinite(o).all() for o in out)
    sum(o.float().sum() for o in out[1:]).backward()
    assert calls == [] and all(p.grad is not None for m in mods for p in m.parameters())
    # the Bernoulli kernel has no gradient for x: a caller who wants one gets it from the composition
    (_, ber, _), x = _ends(torch.float32)
    x.requires_grad_()
    z = torch.randn(15, 4, device="cuda")
    ber.log_prob(x, z).sum().backward()
    assert calls == [] and x.grad is not None and float(x.grad.abs().sum()) > 0
    with torch.no_grad():
        ber.log_prob(x, z)
    assert calls == ["bernoulli_log_prob"]


# ---------------------------------------------------------------- 8. the container
N_FLOWS = 4


def _model(dtype, prior=None, seed=3):
    torch.manual_seed(seed)
    D = nf.distributions
    flows = [nf.flows.Planar(4, act="leaky_relu") for _ in range(N_FLOWS)]
    model = nf.NormalizingFlowVAE(D.DiagGaussian(4) if prior is None else prior, D.NNDiagGaussian(nn.Linear(6, 8)), flows,
                                  D.NNBernoulliDecoder(nn.Linear(4, 6)))
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(0.5 * torch.randn(p.shape))
    return model.to(dtype).cuda()


def _data(b):
    x = torch.rand(b, 6, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    x[0], x[1] = 0.0, 1.0
    return x


def _container_reference(model, x, eps, dtype, prior_log_prob=None):
    names = [n for n, _ in model.named_parameters()]
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}

    def fn(sd_, x_, eps_):
        out, grads = ref.container_grads(sd_, x_, eps_, N_FLOWS, prior_log_prob)
        return out + tuple(grads[n] for n in names)
    return names, references(fn, dtype, sd, x, eps.cpu())


def _run_container(model, x, s, seed, monkeypatch):
    runs = []
    launch = _lib.planar_radial_stack
    monkeypatch.setattr(_lib, "planar_radial_stack", lambda *a, **kw: runs.append(a[0].shape[0]) or launch(*a, **kw))
    calls = count_calls(monkeypatch)
    torch.manual_seed(seed)
    z, log_q, log_p = model(x, num_samples=s)
    assert runs == [len(x) * s], "the Planar layers are not one launch"
    assert calls == ["encode", "bernoulli_log_prob"]
    (log_q.mean() - log_p.mean()).backward()
    assert sorted(calls[2:]) == ["bernoulli_log_prob_bwd", "encode_bwd"]
    torch.manual_seed(seed)
    eps = torch.randn((len(x), s, 4), dtype=x.dtype, device=x.device)
    return (z, log_q, log_p), eps


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_container_matches_the_restatement(hip, dtype, monkeypatch):
    b, s = 5, 3
    model, x = _model(dtype), cuda(_data(b), dtype)
    out, eps = _run_container(model, x, s, 11, monkeypatch)
    assert out[0].shape == (b, s, 4) and out[1].shape == (b, s) and out[2].shape == (b, s)
    names, (r32, r64) = _container_reference(model, x.cpu(), eps, dtype)
    check_all(out, r32 and r32[:3], r64[:3], dtype, "container")
    for i, (name, p) in enumerate(model.named_parameters()):
        assert name == names[i] and p.grad is not None and float(p.grad.abs().sum()) > 0, name
        check(p.grad, r32 and r32[3 + i], r64[3 + i], dtype, "d/d" + name)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_container_with_a_torch_distributions_prior(hip, dtype, monkeypatch):
    b, s = 5, 3
    g = torch.Generator().manual_seed(8)
    loc = torch.randn(4, generator=g, dtype=torch.float64)
    tril = torch.tril(0.3 * torch.randn(4, 4, generator=g, dtype=torch.float64), -1) + torch.diag(0.5 + torch.rand(4, generator=g, dtype=torch.float64))
    prior = torch.distributions.MultivariateNormal(cuda(loc, dtype), scale_tril=cuda(tril, dtype))
    model, x = _model(dtype, prior), cuda(_data(b), dtype)
    assert not any(n.startswith("prior") for n in model.state_dict())
    out, eps = _run_container(model, x, s, 12, monkeypatch)
    cpu_prior = lambda z: torch.distributions.MultivariateNormal(loc.to(z.dtype), scale_tril=tril.to(z.dtype)).log_prob(z)
    names, (r32, r64) = _container_reference(model, x.cpu(), eps, dtype, cpu_prior)
    check_all(out, r32 and r32[:3], r64[:3], dtype, "container, MultivariateNormal prior")
    for i, (name, p) in enumerate(model.named_parameters()):
        check(p.grad, r32 and r32[3 + i], r64[3 + i], dtype, "d/d" + name)
