"""The image data end caps on the HIP kernels (csrc/logit.hip): nf.transforms.Logit in both directions, its accumulating
forms, its VJPs, the byte ingest and a small multiscale Glow behind it, against the plain-torch restatement
(logit_ref.py).

The error rule.  No fixed fp32 tolerance: per tensor, with ref64 the fp64 restatement and ref32 the fp32 restatement on the
same device,

    |kernel - ref64| <= 4 * max|ref32 - ref64| + 8 eps (1 + |ref64|)        over the finite entries,

the factor and the floor allowing for two ``log`` calls of another libm and a differently ordered row sum; the entries
that are not finite must be those of ref32, with its values.  In fp64 the kernel is within 1e-12 (1 + |ref64|) of the fp64
restatement.  Every figure is printed before it is asserted (``LOGIT`` lines)."""
import functools
import math

import pytest
import torch

import logit_ref as ref
import vcnf_amd as nf
from helpers import parity
from vcnf_amd import _lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
# (5, 3, 8, 8): 64 lanes, two workgroups; (3, 3, 32, 32): the real row, 12 trips of a 64-lane group; (7, 1): a lane per
# row; (4, 4099): odd length, scalar accesses, ragged last trip; (1031, 6): 8-byte packs, two lanes (fp32) per row, nine
# workgroups with a ragged last one; (0, 3, 8, 8): no launch
SHAPES = [(5, 3, 8, 8), (3, 3, 32, 32), (7, 1), (4, 4099), (1031, 6), (0, 3, 8, 8)]
ALPHAS = [0.05, 1e-6, 0.0]
EPS = {torch.float32: torch.finfo(torch.float32).eps, torch.float64: torch.finfo(torch.float64).eps}


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v).replace("torch.", "")


@functools.lru_cache(maxsize=None)
def density_input(shape):
    """rand with element 0 of every row 0 and element 1 (where there is one) 1; fp64, CPU."""
    g = torch.Generator().manual_seed(1000 + sum(shape))
    x = torch.rand(shape, dtype=torch.float64, generator=g)
    flat = x.view(len(x), math.prod(shape[1:]))
    flat[:, 0] = 0.0
    if flat.shape[1] > 1:
        flat[:, 1] = 1.0
    return x


@functools.lru_cache(maxsize=None)
def sampling_input(shape, planted_inf=True):
    g = torch.Generator().manual_seed(2000 + sum(shape))
    z = 4 * torch.randn(shape, dtype=torch.float64, generator=g)
    flat = z.view(-1)
    planted = [88.0, -88.0, 104.0, -104.0] + ([math.inf, -math.inf] if planted_inf else [])
    for i, v in enumerate(planted[:flat.numel()]):
        flat[(i * 7919) % flat.numel()] = v
    return z


def held(got, r32, r64, dtype, what):
    """The error rule of the module docstring for one tensor."""
    got, r32, r64 = got.detach().double().cpu(), r32.detach().double().cpu(), r64.detach().double().cpu()
    assert got.shape == r64.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(r64.shape))
    assert not torch.isnan(got).any() or torch.isnan(r32).any(), what + ": NaN"
    ok = torch.isfinite(r64) & torch.isfinite(r32)
    assert torch.equal(torch.isfinite(got), torch.isfinite(r32)), what + ": the entries that are not finite differ"
    assert torch.equal(got[~torch.isfinite(r32)], r32[~torch.isfinite(r32)]), what + ": infinities differ"
    if not ok.any():
        return
    err = (got[ok] - r64[ok]).abs()
    if dtype == torch.float64:
        bound = 1e-12 * (1 + r64[ok].abs())
        noise = 0.0
    else:
        noise = float((r32[ok] - r64[ok]).abs().max())
        bound = 4 * noise + 8 * EPS[dtype] * (1 + r64[ok].abs())
    worst = int((err - bound).argmax())
    print("LOGIT %-52s max err %.3e  fp32 restatement's %.3e  tightest: err %.3e bound %.3e" % (
        what, float(err.max()), noise, float(err[worst]), float(bound[worst])))
    assert bool((err <= bound).all()), "%s: err %.3e > bound %.3e (restatement's fp32 error %.3e)" % (
        what, float(err[worst]), float(bound[worst]), noise)


def restated(direction, alpha, point64, dtype):
    """(ref32 on the device, ref64 on the device) of LogitRef(alpha).<direction>."""
    t = ref.LogitRef(alpha)
    r64 = getattr(t, direction)(point64.cuda())
    r32 = getattr(t, direction)(point64.to(torch.float32).cuda()) if dtype == torch.float32 else r64
    return r32, r64


# ---------------------------------------------------------------- the two directions
@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("alpha", ALPHAS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_inverse_against_the_restatement(hip, shape, alpha, dtype):
    x64 = density_input(shape)
    # fp32 inputs are the rounded fp64 ones: the fp64 restatement sees what the kernel sees
    x = x64.to(dtype).cuda()
    t = nf.transforms.Logit(alpha)
    z, ld = t.inverse(x)
    assert z.shape == x.shape and z.dtype == dtype and ld.shape == (shape[0],) and ld.dtype == dtype
    z2, ld2 = t.inverse(x)
    assert torch.equal(z, z2) and torch.equal(ld, ld2)
    (z32, ld32), (z64, ld64) = restated("inverse", alpha, x.double().cpu(), dtype)
    held(z, z32, z64, dtype, "inverse z %s alpha %g" % (shape, alpha))
    held(ld, ld32, ld64, dtype, "inverse log_det %s alpha %g" % (shape, alpha))
    if alpha == 0.0 and shape[0]:
        assert not torch.isnan(z).any() and not torch.isnan(ld).any()
        assert bool((z.view(shape[0], -1)[:, 0] == -math.inf).all()) and bool((ld == math.inf).all())
        if z[0].numel() > 1:
            assert bool((z.view(shape[0], -1)[:, 1] == math.inf).all())
    elif shape[0]:
        assert torch.isfinite(z).all() and torch.isfinite(ld).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("alpha", [0.05, 1e-6], ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_against_the_restatement(hip, shape, alpha, dtype):
    z = sampling_input(shape).to(dtype).cuda()
    t = nf.transforms.Logit(alpha)
    y, ld = t.forward(z)
    assert y.shape == z.shape and y.dtype == dtype and ld.shape == (shape[0],) and ld.dtype == dtype
    y2, ld2 = t(z)
    assert torch.equal(y, y2) and torch.equal(ld, ld2)
    (y32, ld32), (y64, ld64) = restated("forward", alpha, z.double().cpu(), dtype)
    held(y, y32, y64, dtype, "forward y %s alpha %g" % (shape, alpha))
    held(ld, ld32, ld64, dtype, "forward log_det %s alpha %g" % (shape, alpha))
    assert not torch.isnan(y).any() and not torch.isnan(ld).any()
    if z.numel() >= 6:
        assert int((ld == -math.inf).sum()) >= 1 and torch.isfinite(y).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_the_access_width_does_not_show_in_the_bits(hip, dtype):
    """The same rows behind a pointer that only allows scalar accesses give the bits of the 16-byte packs."""
    t = nf.transforms.Logit(0.05)
    shape = (5, 3, 8, 8)
    x = density_input(shape).to(dtype).cuda()
    z = sampling_input(shape, False).to(dtype).cuda()
    n = x.numel()
    for point, direction in ((x, t.inverse), (z, t.forward)):
        shifted = torch.empty(n + 1, dtype=dtype, device="cuda")[1:].view(shape)
        shifted.copy_(point)
        assert shifted.is_contiguous() and shifted.data_ptr() % 16 != 0
        (a, a_ld), (b, b_ld) = direction(point), direction(shifted)
        assert torch.equal(a, b) and torch.equal(a_ld, b_ld)
    x_u8 = (density_input(shape) * 255).to(torch.uint8).cuda()
    noise = torch.rand(shape, dtype=dtype, device="cuda")
    shifted = torch.empty(n + 1, dtype=torch.uint8, device="cuda")[1:].view(shape)
    shifted.copy_(x_u8)
    (a, a_ld), (b, b_ld) = t.inverse_u8(x_u8, noise, dtype=dtype), t.inverse_u8(shifted, noise, dtype=dtype)
    assert torch.equal(a, b) and torch.equal(a_ld, b_ld)


# ---------------------------------------------------------------- launches, accumulating forms, the walk
class _Launches:
    """Names and arguments of the entry points called while it is active."""

    def __init__(self, monkeypatch):
        self.calls = []
        inner = _lib._launch

        def launch(name, *args):
            self.calls.append((name, args))
            return inner(name, *args)
        monkeypatch.setattr(_lib, "_launch", launch)

    def names(self):
        return [n for n, _ in self.calls]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_a_direction_is_one_launch_and_the_into_forms_accumulate(hip, dtype, monkeypatch):
    sfx = "_f64" if dtype == torch.float64 else "_f32"
    eps = EPS[dtype]
    t = nf.transforms.Logit(0.05)
    shape = (5, 3, 8, 8)
    x = density_input(shape).to(dtype).cuda()
    z = sampling_input(shape, False).to(dtype).cuda()
    log_q0 = torch.linspace(-3, 3, shape[0], dtype=dtype, device="cuda")
    seen = _Launches(monkeypatch)
    out, ld = t.inverse(x)
    assert seen.names() == ["vcnf_logit_inverse" + sfx]
    log_q = log_q0.clone()
    got = t.inverse_into(x, log_q)
    assert seen.names()[1:] == ["vcnf_logit_inverse" + sfx] and seen.calls[1][1][6] == _lib.LD_ACCUM
    assert torch.equal(got, out)
    want = log_q0 + ld
    assert bool(((log_q - want).abs() <= 4 * eps * (1 + want.abs())).all())

    del seen.calls[:]
    out, ld = t.forward(z)
    log_q = log_q0.clone()
    got = t.forward_into(z, log_q)
    assert seen.names() == ["vcnf_logit_forward" + sfx] * 2 and seen.calls[1][1][6] == _lib.LD_ACCUM
    assert torch.equal(got, out)
    want = log_q0 - ld
    assert bool(((log_q - want).abs() <= 4 * eps * (1 + want.abs())).all())

    del seen.calls[:]
    x_u8 = (density_input(shape) * 255).to(torch.uint8).cuda()
    t.inverse_u8(x_u8, torch.rand(shape, dtype=dtype, device="cuda"), dtype=dtype)
    assert seen.names() == ["vcnf_logit_inverse_u8" + sfx]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_normalizing_flow_reaches_the_logit_through_the_walk(hip, dtype, monkeypatch):
    """A Logit as the last flow: the density pass adds its log-det into log_q inside the kernel (inverse_into), the
    sampling pass subtracts it (forward_into); both equal the model whose last flow is the restatement."""
    d = 6
    q0 = nf.distributions.DiagGaussian(d)
    perm = nf.flows.Permute(d, "swap")
    mine = nf.NormalizingFlow(q0, [perm, nf.transforms.Logit(0.05)]).to(dtype).cuda().eval()
    twin = nf.NormalizingFlow(q0, [perm, ref.LogitRef(0.05)]).to(dtype).cuda().eval()
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(33, d, dtype=torch.float64, generator=g) * 0.98 + 0.01).to(dtype).cuda()
    noise = torch.randn(33, d, dtype=torch.float64, generator=g).to(dtype).cuda()
    seen = _Launches(monkeypatch)
    sfx = "_f64" if dtype == torch.float64 else "_f32"
    with torch.no_grad():
        got = mine.log_prob(x)
        assert seen.names().count("vcnf_logit_inverse" + sfx) == 1
        args = dict(seen.calls)["vcnf_logit_inverse" + sfx]
        assert args[6] == _lib.LD_ACCUM and args[7] == 1.0
        want = twin.log_prob(x)
        del seen.calls[:]
        z, lq = mine.sample_from(noise)
        assert seen.names().count("vcnf_logit_forward" + sfx) == 1
        args = dict(seen.calls)["vcnf_logit_forward" + sfx]
        assert args[6] == _lib.LD_ACCUM and args[7] == -1.0
        z_w, lq_w = twin.sample_from(noise)
    tol = 64 * EPS[dtype]
    for a, b, what in ((got, want, "log_prob"), (z, z_w, "sample"), (lq, lq_w, "log_q")):
        err = float(((a - b).abs() / (1 + b.abs())).max())
        print("LOGIT walk %s %s: %.3e" % (what, _ids(dtype), err))
        assert err <= tol, what


# ---------------------------------------------------------------- VJPs
def _vjp_case(direction, shape, alpha, dtype):
    point64 = density_input(shape).clone() if direction == "inverse" else sampling_input(shape, False).clone()
    if direction == "inverse" and alpha == 0.0:
        point64 = point64 * 0.98 + 0.01
    g = torch.Generator().manual_seed(3000 + sum(shape))
    g_out = torch.randn(shape, dtype=torch.float64, generator=g)
    g_ld = torch.randn(shape[0], dtype=torch.float64, generator=g)
    return point64.to(dtype).double(), g_out.to(dtype).double(), g_ld.to(dtype).double()


def _autograd_of(module, direction, point, g_out, g_ld):
    p = point.clone().requires_grad_()
    out, ld = getattr(module, direction)(p)
    terms = ([(out * g_out).sum()] if g_out is not None else []) + ([(ld * g_ld).sum()] if g_ld is not None else [])
    return torch.autograd.grad(sum(terms), p)[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("alpha", [0.05, 1e-6], ids=_ids)
@pytest.mark.parametrize("direction", ["inverse", "forward"])
@pytest.mark.parametrize("shape", [(5, 3, 8, 8), (3, 3, 32, 32), (7, 1), (4, 4099), (1031, 6)], ids=_ids)
def test_vjps_against_autograd_of_the_restatement(hip, shape, direction, alpha, dtype):
    p64, go64, gl64 = _vjp_case(direction, shape, alpha, dtype)
    t, twin = nf.transforms.Logit(alpha), ref.LogitRef(alpha)
    cast = lambda v: None if v is None else v.to(dtype).cuda()
    for which, go, gl in (("both", go64, gl64), ("g_out only", go64, None), ("g_ld only", None, gl64)):
        got = _autograd_of(t, direction, cast(p64), cast(go), cast(gl))
        again = _autograd_of(t, direction, cast(p64), cast(go), cast(gl))
        assert torch.equal(got, again)
        r64 = _autograd_of(twin, direction, p64.cuda(), None if go is None else go.cuda(), None if gl is None else gl.cuda())
        r32 = _autograd_of(twin, direction, cast(p64), cast(go), cast(gl)) if dtype == torch.float32 else r64
        held(got, r32, r64, dtype, "%s vjp %s %s alpha %g" % (direction, which, shape, alpha))


@pytest.mark.parametrize("direction", ["inverse", "forward"])
def test_gradcheck_fp64(hip, direction):
    g = torch.Generator().manual_seed(21)
    t = nf.transforms.Logit(0.05)
    if direction == "inverse":
        p = torch.rand(3, 5, dtype=torch.float64, generator=g) * 0.9 + 0.05
    else:
        p = 2 * torch.randn(3, 5, dtype=torch.float64, generator=g)
    p = p.cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda v: getattr(t, direction)(v), (p,))


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_one_node_with_a_one_launch_backward_and_none_for_data(hip, dtype, monkeypatch):
    sfx = "_f64" if dtype == torch.float64 else "_f32"
    t = nf.transforms.Logit(0.05)
    shape = (5, 3, 8, 8)
    x = density_input(shape).to(dtype).cuda()
    z = sampling_input(shape, False).to(dtype).cuda()
    seen = _Launches(monkeypatch)
    for point, direction, stem in ((x, "inverse", "vcnf_logit_inverse"), (z, "forward", "vcnf_logit_forward")):
        out, ld = getattr(t, direction)(point)                # data: no node
        assert out.grad_fn is None and ld.grad_fn is None and not out.requires_grad and not ld.requires_grad
        p = point.clone().requires_grad_()
        del seen.calls[:]
        out, ld = getattr(t, direction)(p)
        assert out.grad_fn is not None and out.grad_fn.name() == ld.grad_fn.name() == "LogitFnBackward", "one node"
        assert seen.names() == [stem + sfx]
        (out.sum() + ld.sum()).backward()
        assert seen.names() == [stem + sfx, stem + "_bwd" + sfx] and p.grad.shape == p.shape
        # the accumulating form of a tensor that requires grad: the same values, differentiable
        q = point.clone().requires_grad_()
        log_q = torch.zeros(shape[0], dtype=dtype, device="cuda")
        got = getattr(t, direction + "_into")(q, log_q)
        assert torch.equal(got, out) and torch.equal(log_q, ld if direction == "inverse" else -ld)
        (got.sum() + (log_q.sum() if direction == "inverse" else -log_q.sum())).backward()
        assert torch.equal(q.grad, p.grad)


# ---------------------------------------------------------------- bytes
def _all_bytes():
    return torch.arange(256, dtype=torch.uint8).repeat(3)[torch.randperm(768, generator=torch.Generator().manual_seed(5))].reshape(4, 3, 8, 8)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("alpha", [0.05, 1e-6], ids=_ids)
def test_inverse_u8_against_the_chain(hip, alpha, dtype):
    x_u8 = _all_bytes()
    assert len(torch.unique(x_u8)) == 256
    t = nf.transforms.Logit(alpha)
    last = math.nextafter(1.0, 0.0) if dtype == torch.float64 else float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    g = torch.Generator().manual_seed(6)
    for what, noise in (("noise 0", torch.zeros(x_u8.shape, dtype=dtype)), ("noise 1-", torch.full(x_u8.shape, last, dtype=dtype)),
                        ("noise rand", torch.rand(x_u8.shape, dtype=dtype, generator=g))):
        assert float(noise.max()) < 1.0
        z, ld = t.inverse_u8(x_u8.cuda(), noise.cuda(), dtype=dtype)
        assert z.dtype == dtype and z.shape == x_u8.shape and ld.shape == (4,)
        z64, ld64 = ref.inverse_u8(x_u8.cuda(), noise.double().cuda(), alpha)
        z32, ld32 = ref.inverse_u8(x_u8.cuda(), noise.cuda(), alpha)
        held(z, z32, z64, dtype, "inverse_u8 z %s alpha %g" % (what, alpha))
        held(ld, ld32, ld64, dtype, "inverse_u8 log_det %s alpha %g" % (what, alpha))
        assert torch.isfinite(z).all() and torch.isfinite(ld).all()
        # the chain is evaluated one rounded operation at a time: the x the kernel forms is the composition's, taken on
        # the CPU, where torch divides by 255 (on the device it multiplies by the rounded reciprocal)
        x = ref.bytes_to_unit(x_u8, noise)
        z_x, ld_x = t.inverse(x.cuda())
        assert torch.equal(z, z_x) and torch.equal(ld, ld_x), what + ": not the bits of inverse(bytes -> jitter -> scale)"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_inverse_u8_draws_its_noise_with_one_torch_rand(hip, dtype):
    x_u8 = _all_bytes().cuda()
    t = nf.transforms.Logit(0.05)
    torch.manual_seed(123)
    z, ld = t.inverse_u8(x_u8, dtype=dtype)
    after = torch.rand(3, device="cuda")
    torch.manual_seed(123)
    z_w, ld_w = t.inverse_u8(x_u8, noise=torch.rand(x_u8.shape, dtype=dtype, device="cuda"), dtype=dtype)
    assert z.dtype == dtype and torch.equal(z, z_w) and torch.equal(ld, ld_w)
    assert torch.equal(after, torch.rand(3, device="cuda")), "more than one draw"


# ---------------------------------------------------------------- the model
NC = 4


def _glow(transforms, seed=31):
    """A two-level multiscale Glow on 3 x 8 x 8 (one GlowBlock per level, hidden 16, GlowBase bases), once per transform
    over the SAME flow and base modules.  The parameters are moved off their initial values; the ActNorms count as
    initialised."""
    levels, hidden, inp = 2, 16, (3, 8, 8)
    merges, flows, shapes = [], [], []
    for i in range(levels):
        flows += [[nf.flows.GlowBlock(inp[0] * 2 ** (levels + 1 - i), hidden, split_mode="channel", scale=True), nf.flows.Squeeze()]]
        if i > 0:
            merges += [nf.flows.Merge()]
            shapes += [(inp[0] * 2 ** (levels - i), inp[1] // 2 ** (levels - i), inp[2] // 2 ** (levels - i))]
        else:
            shapes += [(inp[0] * 2 ** (levels + 1), inp[1] // 2 ** levels, inp[2] // 2 ** levels)]
    q0 = [nf.distributions.GlowBase(s, NC) for s in shapes]
    models = [nf.MultiscaleFlow(q0, flows, merges, transform=t, class_cond=True).cuda() for t in transforms]
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in models[0].parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=g).to(p.device))
        for m in models[0].modules():
            if isinstance(m, nf.flows.ActNorm):
                m.data_dep_init_done.fill_(1.0)
    for m in models:
        m.refresh_packed()
    return models, shapes


def _images(n, seed=41):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(256, (n, 3, 8, 8), generator=g).to(torch.uint8), torch.randint(NC, (n,), generator=g), g


def test_multiscale_glow_behind_the_transform(hip):
    (mine, twin), shapes = _glow([nf.transforms.Logit(0.05), ref.LogitRef(0.05)])
    assert [tuple(p.shape) for p in mine.parameters()] == [tuple(p.shape) for p in twin.parameters()]
    x_u8, y, g = _images(8)
    x_u8, y = x_u8.cuda(), y.cuda()
    noise_u = torch.rand(x_u8.shape, generator=g).cuda()
    x = ref.bytes_to_unit(x_u8, noise_u)
    mine.eval(), twin.eval()
    with torch.no_grad():
        got, want = mine.log_prob(x, y), twin.log_prob(x, y).cpu()
        assert torch.isfinite(want).all()
        parity(got, want, want.double(), what="log_prob behind Logit")
        noise = [torch.randn(8, *s, generator=g).cuda() for s in shapes]
        (z, lq), (z_w, lq_w) = mine.sample_from(noise, y), twin.sample_from(noise, y)
        assert torch.isfinite(z_w).all() and bool((z_w > -0.06).all()) and bool((z_w < 1.06).all())
        parity(z, z_w.cpu(), z_w.double().cpu(), what="sample_from behind Logit")
        parity(lq, lq_w.cpu(), lq_w.double().cpu(), what="log_q behind Logit")
        # bytes: the model draws the dequantisation noise itself, in the dtype of the first base's loc
        torch.manual_seed(9)
        from_bytes = mine.log_prob(x_u8, y)
        torch.manual_seed(9)
        drawn = torch.rand(x_u8.shape, dtype=torch.float32, device="cuda")
        chain = mine.log_prob(ref.bytes_to_unit(x_u8, drawn), y).cpu()
        assert from_bytes.dtype == torch.float32 and torch.isfinite(chain).all()
        parity(from_bytes, chain, chain.double(), what="log_prob(uint8) against the float chain")
        torch.manual_seed(9)
        assert torch.equal(-mine.forward_kld(x_u8, y), from_bytes.mean())
    grads = []
    for model in (mine, twin):
        model.train()
        for p in model.parameters():
            p.grad = None
        loss = model.forward_kld(x, y)
        assert loss.grad_fn is not None
        loss.backward()
        grads.append([None if p.grad is None else p.grad.detach().cpu().clone() for p in model.parameters()])
    assert sum(a is not None for a in grads[0]) > 10
    for (name, _), a, b in zip(mine.named_parameters(), *grads):
        assert (a is None) == (b is None), name
        if a is not None:
            parity(a, b, b.double(), what="d forward_kld / d " + name)


def test_multiscale_glow_refuses_bytes_without_a_logit(hip):
    (plain, shifted), _ = _glow([None, nf.transforms.Shift(0.5)])
    x_u8, y, _ = _images(4)
    for model, word in ((plain, "None"), (shifted, "Shift")):
        with pytest.raises(TypeError, match=word):
            model.log_prob(x_u8.cuda(), y.cuda())


# ---------------------------------------------------------------- graph capture
def test_the_directions_and_the_byte_ingest_are_capturable(hip):
    """inverse, forward and inverse_u8 (noise given) under torch.cuda.graph (one stream, side-stream warm-up as
    vcnf_amd.graphs does): new data copied into the static buffers, replay has the eager call's bits."""
    t = nf.transforms.Logit(0.05)
    shape = (33, 3, 8, 8)
    g = torch.Generator().manual_seed(51)

    def draw():
        return (torch.rand(shape, generator=g).cuda(), (4 * torch.randn(shape, generator=g)).cuda(),
                torch.randint(256, shape, generator=g).to(torch.uint8).cuda(), torch.rand(shape, generator=g).cuda())

    def run(x, z, x_u8, noise):
        return t.inverse(x) + t.forward(z) + t.inverse_u8(x_u8, noise)
    static = draw()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            run(*static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = run(*static)
    for _ in range(2):
        fresh = draw()
        for a, b in zip(static, fresh):
            a.copy_(b)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = run(*fresh)
        assert all(torch.isfinite(e).all() and torch.equal(o, e) for o, e in zip(out, eager))
