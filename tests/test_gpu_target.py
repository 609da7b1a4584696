"""The target densities on the GPU (csrc/target_density.hip through vcnf_amd.distributions.target and NormalizingFlow)
against the plain-torch restatement target_ref.py run on the CPU.  fp32 results are judged by helpers.parity against the
restatement's fp32 run with its own fp32-vs-fp64 noise as the yardstick (every batch here has fewer than 2048 rows, so
the noise of the B = 1000 case of the same target is passed as noise_floor to the smaller ones), fp64 results by
assert_close at 1e-10 (gradients: 1e-9 of the tensor's largest entry).

The batches are a single row (the r == 0 row), a partial wave, an exact wave, a wave + 1 and a partial last workgroup;
the component counts include 1, an odd one and one above the eight of the default."""
import functools

import pytest
import torch

import target_ref as ref
import vcnf_amd as nf
from helpers import assert_close, parity
from vcnf_amd import _lib
from vcnf_amd.flows import Planar

pytestmark = pytest.mark.gpu

CASES = [("two_moons", 0), ("circular", 2), ("circular", 8), ("circular", 33), ("ring", 1), ("ring", 2), ("ring", 7)]
DEFAULTS = [("two_moons", 0), ("circular", 8), ("ring", 2)]
REJECTION = [("two_moons", 0), ("ring", 2)]              # the targets that sample by rejection
BATCHES = [1, 63, 64, 65, 1000]
DTYPES = [torch.float32, torch.float64]
IDS = ["fp32", "fp64"]
F64 = dict(rtol=1e-10, atol=1e-10)
TIE_SHARE = 0.002
case_id = lambda c: "%s-%d" % c if isinstance(c, tuple) else str(c)


def target_of(family, n, dtype):
    """The module on the GPU; fp64 through .double() as a user converts a model."""
    D = nf.distributions
    t = D.TwoMoons() if family == "two_moons" else D.CircularGaussianMixture(n) if family == "circular" else D.RingMixture(n)
    return (t.double() if dtype == torch.float64 else t).cuda()


@functools.lru_cache(maxsize=None)
def reference(family, n, b):
    """The restatement on the CPU in fp32 and fp64 for one case: {dtype: (log p, score, d (g . log p) / d z, log p with
    the NaN row appended)}, and the inputs.  Shared between tests: do not modify."""
    z, g, _, _ = ref.inputs(family, n, b)
    out = {"z": z, "g": g}
    for dtype in DTYPES:
        lp, score, grad = ref.gradients(family, n, z, g, dtype)
        with torch.no_grad():
            lp_nan = ref.log_prob(family, n, ref.nan_row(z.to(dtype)))
        assert torch.isfinite(lp).all() and torch.isfinite(score).all() and torch.isfinite(grad).all()
        assert torch.isnan(lp_nan[-1]) and torch.equal(lp_nan[:-1], lp)
        out[dtype] = (lp, score, grad, lp_nan)
    return out


def floors(family, n, b):
    """noise_floor per quantity from the B = 1000 case of the same target (0 for that case itself)."""
    if b == 1000:
        return (0.0, 0.0, 0.0, 0.0)
    big = reference(family, n, 1000)
    return tuple(float((big[torch.float32][j].double() - big[torch.float64][j])[:1000].abs().max()) for j in range(4))


def largest(family, n, j):
    """The largest entry of quantity ``j`` in the B = 1000 case of a target: what "1e-9 of the tensor's largest entry"
    refers to for the smaller batches of the same target, as noise_floor does for fp32.  A small batch can be all
    cancellation: the single row (0, 0) of a circular mixture has the score 0 by symmetry, the sum of n terms of size
    2 / (n scale^2) (3.8 for 8 modes), so both sides hold roundings of those terms, 1e-15, and nothing to scale by."""
    return float(reference(family, n, 1000)[torch.float64][j].abs().max())


def judge(got, r, j, dtype, what, noise_floor=0.0, gradient=False, largest_entry=0.0):
    r32, r64 = r[torch.float32][j], r[torch.float64][j]
    got = got.detach().cpu()
    assert got.dtype == dtype and got.shape == r64.shape, what
    if dtype == torch.float32:
        parity(got, r32, r64, what=what, noise_floor=noise_floor)
    elif gradient:
        bound = 1e-9 * max(float(r64.abs().max()), largest_entry)
        err = float((got - r64).abs().max())
        assert torch.isfinite(got).all() and err <= bound, "%s: %.3e > %.3e" % (what, err, bound)
    else:
        assert_close(got, r64, what=what, **F64)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_log_prob_score_and_gradient(hip, case, dtype):
    family, n = case
    target = target_of(family, n, dtype)
    for b in BATCHES:
        r = reference(family, n, b)
        nf_lp, nf_score, nf_grad, nf_nan = floors(family, n, b)
        tag = "%s n=%d B=%d %s" % (family, n, b, dtype)
        z = r["z"].to(dtype).cuda()
        with torch.no_grad():
            lp = target.log_prob(z)
            score = target.score(z)
            lp_nan = target.log_prob(ref.nan_row(z))
            score_nan = target.score(ref.nan_row(z))
        x = z.clone().requires_grad_(True)
        lp_graph = target.log_prob(x)
        assert lp_graph.grad_fn is not None and type(lp_graph.grad_fn).__name__.startswith("TargetLogProbFn")   # ONE node
        grad, = torch.autograd.grad((r["g"].to(dtype).cuda() * lp_graph).sum(), x)
        for j, (name, t) in enumerate((("log_prob", lp), ("score", score), ("gradient", grad))):
            err, noise = ((x.detach().cpu().double() - r[torch.float64][j]).abs().max() for x in (t, r[torch.float32][j]))
            print("%s %s: max |got - fp64 restatement| %.3e (the fp32 restatement's %.3e)" % (tag, name, float(err), float(noise)))
        judge(lp, r, 0, dtype, tag + " log_prob", nf_lp)
        judge(score, r, 1, dtype, tag + " score", nf_score, gradient=True, largest_entry=largest(family, n, 1))
        judge(grad, r, 2, dtype, tag + " gradient", nf_grad, gradient=True, largest_entry=largest(family, n, 2))
        judge(lp_nan, r, 3, dtype, tag + " log_prob with a NaN row", nf_nan)
        assert torch.equal(lp_graph.detach(), lp), tag + ": log_prob differs under autograd"
        assert torch.equal(lp_nan[:-1], lp) and bool(torch.isnan(lp_nan[-1])) and bool(torch.isnan(score_nan[-1]).all())
        assert torch.equal(score_nan[:-1], score)
        # the r == 0 row: finite, and where the density depends on z through r and |z0| alone, exactly the restatement's 0
        assert r["z"][0].tolist() == [0.0, 0.0] and torch.isfinite(score[0]).all() and torch.isfinite(grad[0]).all()
        if family != "circular":
            assert score[0].tolist() == r[torch.float64][1][0].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_misaligned_rows_and_scoreless_path(hip, case, dtype):
    """z one element past its allocation takes the element loads; the launch without a score is another kernel instance.
    Both give the bits of the aligned launch with a score."""
    family, n = case
    target = target_of(family, n, dtype)
    for b in (65, 1000):
        z = reference(family, n, b)["z"].to(dtype).cuda()
        buf = torch.empty(2 * b + 1, dtype=dtype, device="cuda")
        buf[1:] = z.reshape(-1)
        shifted = buf[1:2 * b + 1].view(b, 2)
        width = 2 * z.element_size()
        assert shifted.is_contiguous() and z.data_ptr() % width == 0 and shifted.data_ptr() % width == z.element_size()
        table, scale = target._operands(z)
        with torch.no_grad():
            lp, score = _lib.target_log_prob(z, target._family, table, scale, want_score=True)
            lp_plain, none = _lib.target_log_prob(z, target._family, table, scale)
            lp_shift, score_shift = _lib.target_log_prob(shifted, target._family, table, scale, want_score=True)
            lp_shift_plain, _ = _lib.target_log_prob(shifted, target._family, table, scale)
            assert none is None and torch.isfinite(lp).all()
            assert torch.equal(lp, lp_plain), "log_prob depends on whether the score is written"
            assert torch.equal(lp, lp_shift) and torch.equal(score, score_shift) and torch.equal(lp, lp_shift_plain)
            assert torch.equal(target.log_prob(shifted), lp) and torch.equal(target.score(shifted), score)
            # a non-contiguous view is made contiguous
            wide = torch.zeros(b, 4, dtype=dtype, device="cuda")
            wide[:, 1:3] = z
            assert torch.equal(target.log_prob(wide[:, 1:3]), lp)


def test_bad_inputs_raise(hip):
    for family, n in DEFAULTS:
        target = target_of(family, n, torch.float32)
        for bad in (torch.zeros(4, 3, device="cuda"), torch.zeros(4, device="cuda"), torch.zeros(4, 2, 1, device="cuda"),
                    torch.zeros(4, 2, device="cuda", dtype=torch.float16), torch.zeros(4, 2, device="cuda", dtype=torch.int64),
                    torch.zeros(4, 2)):
            for call in (target.log_prob, target.score):
                with pytest.raises(nf.VcnfError):
                    call(bad)
        empty = torch.zeros(0, 2, device="cuda")
        assert tuple(target.log_prob(empty).shape) == (0,) and tuple(target.score(empty).shape) == (0, 2)


# ---------------------------------------------------------------- rejection sampling
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", REJECTION, ids=case_id)
def test_acceptance_mask(hip, case, dtype):
    family, n = case
    target = target_of(family, n, dtype)
    _, _, eps, u = ref.inputs(family, n, 1000)
    z64, want, near = ref.accept(family, n, eps, u)
    assert float(near.double().mean()) <= TIE_SHARE
    z_, accept = target._accept(eps.to(dtype).cuda(), u.to(dtype).cuda())
    assert z_.dtype == dtype and accept.dtype == torch.bool and tuple(accept.shape) == (ref.DRAWS,)
    assert_close(z_, z64, rtol=0.0, atol=4 * torch.finfo(dtype).eps * 3.0, what="proposals")
    differ = (accept.cpu() != want) & ~near
    assert not differ.any(), "%d draws outside the tie band are decided differently" % int(differ.sum())
    assert 0.01 < float(accept.double().mean()) < 0.5


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", REJECTION, ids=case_id)
def test_rejection_sampling_and_sample(hip, case, dtype):
    family, n = case
    target = target_of(family, n, dtype)
    steps = 4096
    for seed in (0, 17):
        torch.manual_seed(seed)
        got = target.rejection_sampling(steps)
        torch.manual_seed(seed)
        eps = torch.rand((steps, 2), dtype=dtype, device="cuda")
        u = torch.rand(steps, dtype=dtype, device="cuda")
        z_, accept = target._accept(eps, u)
        assert got.dtype == dtype and 0 < len(got) < steps and torch.equal(got, z_[accept])
    torch.manual_seed(5)
    z = target.sample(500)
    assert tuple(z.shape) == (500, 2) and z.dtype == dtype == target.prop_scale.dtype and z.is_cuda
    assert torch.isfinite(z).all() and float(z.min()) >= -3.0 and float(z.max()) <= 3.0
    assert tuple(target.sample(1).shape) == (1, 2)


def test_circular_mixture_sample(hip):
    target = target_of("circular", 8, torch.float32)
    torch.manual_seed(23)
    z = target.sample(8000)
    assert tuple(z.shape) == (8000, 2) and z.dtype == torch.float32 and z.is_cuda
    centres = target.table.float()
    nearest = torch.cdist(z, centres).argmin(1)
    counts = torch.bincount(nearest, minlength=8)
    # 5 sigma of a binomial(8000, 1/8): sigma = 29.6
    assert int(counts.sum()) == 8000 and int((counts - 1000).abs().max()) <= 150, counts.tolist()
    std = (z - centres[nearest]).double().std(0)
    scale = float(target.scale)
    assert float((std - scale).abs().max()) <= 0.05 * scale, (std.tolist(), scale)
    assert target.double().sample(10).dtype == torch.float64


# ---------------------------------------------------------------- training
def objectives(act):
    """(name, call): the estimators of the reference's drivers.  Those that evaluate log q of given points with frozen
    parameters (score_fn=False, dreg=True) invert the flows, which Planar does for leaky_relu only - here as in the
    reference.  reverse_alpha_div without dreg is sign(alpha - 1) logsumexp(.): identically 0 at the default alpha = 1,
    so its gradient is asked for at alpha = 0.5 and 2 and only finiteness at the default."""
    out = [("reverse_kld", lambda m: m.reverse_kld(256), True),
           ("reverse_alpha_div alpha=1", lambda m: m.reverse_alpha_div(256, dreg=False), False),
           ("reverse_alpha_div alpha=0.5", lambda m: m.reverse_alpha_div(256, alpha=0.5, dreg=False), True),
           ("reverse_alpha_div alpha=2", lambda m: m.reverse_alpha_div(256, alpha=2, dreg=False), True)]
    if act == "leaky_relu":
        out += [("reverse_kld score_fn=False", lambda m: m.reverse_kld(256, score_fn=False), True),
                ("reverse_alpha_div dreg", lambda m: m.reverse_alpha_div(256, dreg=True), True)]
    return out


@pytest.mark.parametrize("act", ["tanh", "leaky_relu"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", DEFAULTS, ids=case_id)
def test_objectives_train(hip, case, dtype, act):
    family, n = case
    torch.manual_seed(41)
    target = target_of(family, n, torch.float32)
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), [Planar(2, act=act) for _ in range(8)], p=target)
    model = (model.double() if dtype == torch.float64 else model).cuda()
    assert not list(target.parameters())
    assert [k for k in model.state_dict() if k.startswith("p.")] == ["p.prop_scale", "p.prop_shift"] + (["p.scale"] if family == "circular" else [])
    assert all(not k.startswith("p.") for k, _ in model.named_parameters())
    for name, call, moves in objectives(act):
        runs = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(7)
            loss = call(model)
            loss.backward()
            runs.append((loss.detach().clone(), {k: p.grad.clone() for k, p in model.flows.named_parameters()}))
        loss, grads = runs[0]
        tag = "%s %s %s %s" % (family, dtype, act, name)
        assert loss.dtype == dtype and bool(torch.isfinite(loss)), tag
        for k, g in grads.items():
            assert torch.isfinite(g).all(), "%s: d %s" % (tag, k)
            assert not moves or bool((g != 0).any()), "%s: d %s is all zero" % (tag, k)
            assert torch.equal(g, runs[1][1][k]), "%s: d %s differs between two calls under one seed" % (tag, k)
        assert torch.equal(loss, runs[1][0]), tag + ": the loss differs between two calls under one seed"


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", DEFAULTS, ids=case_id)
def test_graph_capture(hip, case, dtype):
    """log_prob at B = 1024 captured on one stream and replayed on another z equals the eager result bitwise."""
    family, n = case
    target = target_of(family, n, dtype)
    gen = torch.Generator().manual_seed(ref.seed_of("capture", family, n))
    first, second = (2.0 * torch.randn(1024, 2, generator=gen, dtype=torch.float64).to(dtype).cuda() for _ in range(2))
    static = first.clone()
    with torch.no_grad():
        want_first, want_second = target.log_prob(first), target.log_prob(second)      # also casts the table, outside capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            target.log_prob(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = target.log_prob(static)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_first)
        static.copy_(second)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_second) and not torch.equal(want_first, want_second)
