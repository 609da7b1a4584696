"""Planar and Radial flows on the GPU (csrc/planar_radial.hip through vcnf_amd.fused_planar, the modules and
NormalizingFlow) against the plain-torch restatement planar_radial_ref.py run on the CPU.  fp32 results are judged by
helpers.parity against the restatement's fp32 run with its own fp32-vs-fp64 noise as the yardstick, fp64 results by
assert_close at 1e-10 (gradients: 1e-9 of the tensor's largest entry).  Rows whose fp64 trace comes within 1e-4 of a kink
(lin = 0 of a leaky_relu layer, r = 0 of a radial layer) are left out and their cotangents are zero; at most 2 % are.
A layer's one-element gradients take the noise of all the layer's gradient entries as their yardstick (layer_noise), and
the cases with few rows (B = 1, 63, and the deep run) a larger sample of the noise of their own layers (same_case_floor).

The shapes are the smallest at which the lane-group layout (4 features per lane, 1 - 64 lanes per sample), the partial
last workgroup and the layer loop can go wrong; the deep case has more operands than fit in the LDS."""
import functools

import pytest
import torch

import planar_radial_ref as ref
import vcnf_amd as nf
from helpers import assert_close, parity
from vcnf_amd import _lib, fused_planar
from vcnf_amd.flows import Planar, Radial

pytestmark = pytest.mark.gpu

SHAPES = [1, 2, 3, 5, 16, 17, 64, 65, 130, (2, 3, 3)]
RUNS = [(1, 64), (2, 65), (33, 1000), (33, 1), (33, 63)]
STACKS = ["tanh", "leaky_relu", "radial", "mixed"]
DEEP = (200, 130, 65)                     # K, D, B: 210 KB of fp32 operands
DTYPES = [torch.float32, torch.float64]
F64 = dict(rtol=1e-10, atol=1e-10)


def tup(shape):
    return (shape,) if isinstance(shape, int) else tuple(shape)


def module_of(p, shape, dtype):
    if p["kind"] == "radial":
        f = Radial(shape, z_0=p["z_0"].to(dtype))
        f.alpha.data = p["alpha"].to(dtype)
        f.beta.data = p["beta"].to(dtype)
        return f
    return Planar(shape, act=p["kind"], u=p["u"].to(dtype), w=p["w"].to(dtype), b=p["b"].to(dtype))


def model_of(layers, shape, dtype):
    flows = [module_of(p, shape, dtype) for p in layers]
    return nf.NormalizingFlow(nf.distributions.DiagGaussian(tup(shape)), flows).to(dtype).cuda()


@functools.lru_cache(maxsize=None)
def reference(stack, shape, k, b):
    """The restatement on the CPU in fp32 and fp64 for one case: forward results, gradients for both cotangents, the
    rows kept and the cotangents with the other rows zeroed.  Shared between tests: do not modify."""
    layers, z, g_z, g_ld = ref.inputs(stack, shape, k, b)
    with torch.no_grad():
        _, _, trace = ref.forward(z, layers)
    keep = ~ref.kink_rows(trace, layers)
    assert int((~keep).sum()) <= 0.02 * b, "%d of %d rows near a kink" % (int((~keep).sum()), b)
    g_z, g_ld = g_z.clone(), g_ld.clone()
    g_z[~keep] = 0
    g_ld[~keep] = 0
    out = {"layers": layers, "z": z, "g_z": g_z, "g_ld": g_ld, "keep": keep}
    for dtype in DTYPES:
        res = ref.gradients(layers, z, g_z, g_ld, dtype)
        for t in res[:4]:
            assert torch.isfinite(t).all()
        assert all(torch.isfinite(g).all() for layer in res[4] for g in layer.values())
        out[dtype] = res
    return out


def judge(got, r, dtype, pick, what, rows=None, noise_floor=0.0):
    """``got`` against the restatement's result ``pick(r[dtype])``, on the rows kept when it is per sample."""
    r32, r64 = pick(r[torch.float32]), pick(r[torch.float64])
    got = got.detach().cpu()
    if rows is not None:
        got, r32, r64 = got[rows], r32[rows], r64[rows]
    if dtype == torch.float32:
        parity(got, r32, r64, what=what, noise_floor=noise_floor)
    else:
        assert_close(got, r64, what=what, **F64)


def log_q_of(r, dtype):
    """log q of sample_from at the base draw z: the standard normal's log density minus the log-dets."""
    return ref.gaussian_log_prob(r["z"].to(dtype)) - r[dtype][1]


def check_forward(stack, shape, k, b, dtype, floor=None):
    r = reference(stack, shape, k, b)
    model = model_of(r["layers"], shape, dtype)
    eps = r["z"].to(dtype).cuda()
    lq = {d: log_q_of(r, d) for d in DTYPES}
    nz, nl = (floor["z"], floor["log_q"]) if floor else (0.0, 0.0)
    tag = "%s %s K=%d B=%d %s" % (stack, shape, k, b, dtype)
    with torch.no_grad():
        assert fused_planar.plan(list(model.flows), 0, eps, False)[0] == k
        z1, q1 = model.sample_from(eps)
        z2, q2 = model.sample_from(eps)
        assert torch.equal(z1, z2) and torch.equal(q1, q2), tag + ": the same call twice differs"
        model.fuse_planar_stacks = False
        z3, q3 = model.sample_from(eps)
    for name, z, q in (("run", z1, q1), ("layer by layer", z3, q3)):
        judge(z, r, dtype, lambda t: t[0], "%s z (%s)" % (tag, name), r["keep"], nz)
        judge(q, {d: (lq[d],) for d in DTYPES}, dtype, lambda t: t[0], "%s log_q (%s)" % (tag, name), r["keep"], nl)


@pytest.mark.parametrize("stack", STACKS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_run(hip, shape, stack):
    """sample_from through the run and layer by layer, fp32 and fp64, at every (K, B)."""
    for dtype in DTYPES:
        for k, b in RUNS:
            check_forward(stack, shape, k, b, dtype, floor=same_case_floor(stack, shape, k, b) if needs_floor(k, b) else None)


@pytest.mark.parametrize("stack", ["tanh", "radial"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_forward_deep_run(hip, stack, dtype):
    """More layer operands than the LDS holds."""
    k, d, b = DEEP
    check_forward(stack, d, k, b, dtype, floor=same_case_floor(stack, d, k, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_ld_modes_through_the_wrapper(hip, dtype):
    """Accumulating into a running log_q with sign -1 agrees with the stored value to one rounding."""
    for stack, shape, k, b in (("mixed", 5, 33, 63), ("leaky_relu", 17, 2, 65)):
        r = reference(stack, shape, k, b)
        model = model_of(r["layers"], shape, dtype)
        z = r["z"].to(dtype).cuda()
        with torch.no_grad():
            codes, va, vb, sc = fused_planar.operands(list(model.flows), z.device, dtype)
            out, ld = _lib.planar_radial_stack(z, codes, va, vb, sc)
            base = torch.randn(b, dtype=dtype, device="cuda")
            out2, acc = _lib.planar_radial_stack(z, codes, va, vb, sc, logdet=base.clone(), sign=-1.0)
            _, neg = _lib.planar_radial_stack(z, codes, va, vb, sc, sign=-1.0)
        assert torch.equal(out, out2) and torch.equal(neg, -ld)
        eps = torch.finfo(dtype).eps
        assert_close(acc, base - ld, rtol=eps, atol=eps, what="accumulated log_q")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_single_layers(hip, shape):
    """A layer's forward is the kernel with K = 1; the leaky_relu inverse, its run in log_prob and the round trip."""
    b = 65
    for dtype in DTYPES:
        for kind in ref.KINDS:
            r = reference(kind, shape, 1, b)
            layer = module_of(r["layers"][0], shape, dtype).cuda()
            with torch.no_grad():
                out, ld = layer(r["z"].to(dtype).cuda())
            assert out.shape == r["z"].shape and tuple(ld.shape) == (b,)
            judge(out, r, dtype, lambda t: t[0], "%s %s forward z" % (kind, shape), r["keep"])
            judge(ld, r, dtype, lambda t: t[1], "%s %s forward log_det" % (kind, shape), r["keep"])
        r = reference("leaky_relu", shape, 2, b)
        # the inverse meets its kinks on the output side: the rows within KINK of one there are left out as well
        keep = r["keep"] & inverse_keep(r[torch.float64][0], r["layers"])
        assert int((~keep).sum()) <= 0.02 * b
        model = model_of(r["layers"], shape, dtype)
        x = r[torch.float64][0].to(dtype).cuda()
        with torch.no_grad():
            z1, ld1 = model.flows[1].inverse(x)
            z0, ld0 = model.flows[0].inverse(z1)
            lp = model.log_prob(x)
            model.fuse_planar_stacks = False
            lp_layers = model.log_prob(x)
            fwd, _ = model.flows[0](r["z"].to(dtype).cuda())
            trip, ld_trip = model.flows[0].inverse(fwd)
        # the inputs of the inverse differ between the precisions (the fp32 reference inverts its own fp32 output), so
        # fp32 is judged on the fp64 output cast down, against the restatement's inverse of the same tensor
        with torch.no_grad():
            same = {d: ref.inverse(x.cpu().to(d), ref.cast(r["layers"], d)) for d in DTYPES}
            same = {d: (same[d][0], same[d][1], ref.gaussian_log_prob(same[d][0]) + same[d][1]) for d in DTYPES}
        judge(z0, same, dtype, lambda t: t[0], "%s inverse z" % (shape,), keep)
        judge(ld0 + ld1, same, dtype, lambda t: t[1], "%s inverse log_det" % (shape,), keep)
        judge(lp, same, dtype, lambda t: t[2], "%s log_prob (run)" % (shape,), keep)
        judge(lp_layers, same, dtype, lambda t: t[2], "%s log_prob (layer by layer)" % (shape,), keep)
        # round trip through one layer: against the restatement's own round trip in the same precision
        with torch.no_grad():
            p = ref.cast(r["layers"], dtype)[0]
            f_ref, _, lin0 = ref.planar_forward(r["z"].to(dtype), p)
            t_ref, _ = ref.planar_inverse(f_ref, p)
        rows = lin0.double().abs() >= ref.KINK
        err = (trip.cpu() - r["z"].to(dtype))[rows].abs().max()
        err_ref = (t_ref - r["z"].to(dtype))[rows].abs().max()
        assert float(err) <= 4.0 * float(err_ref) + (1e-6 if dtype == torch.float32 else 1e-12), (shape, dtype, float(err), float(err_ref))


def inverse_keep(x, layers):
    """[B] bool: rows of the fp64 inverse pass from x that stay KINK away from lin = 0 in every layer."""
    keep = torch.ones(len(x), dtype=torch.bool)
    with torch.no_grad():
        for p in reversed(layers):
            keep &= (ref._sum(p["w"] * x) + p["b"]).abs() >= ref.KINK
            x, _ = ref.planar_inverse(x, p)
    return keep


def layer_noise(r, i):
    """The restatement's fp32-vs-fp64 noise over all gradient entries of layer ``i``: the yardstick for the layer's
    one-element gradients (b; alpha, beta).  parity measures the noise on the tensor it compares, and on a single element
    that is one draw of the rounding error, which can come out far below its typical size (helpers.parity's noise_floor
    is there for this).  The same layer's other gradients come through the same chain of later layers and have the same
    conditioning, so their largest error is the sample the one element is judged by.  On the MI355X d b of layer 34 of
    the 200 tanh layers was off by 4.5e-3 of 75, 6e-5 relative, where the restatement's own fp32 run happened to be
    within 1.2e-6 relative at that element and 6e-6 to 8e-5 relative at the b of the layers around it."""
    return max(float((r[torch.float32][4][i][n].double() - r[torch.float64][4][i][n]).abs().max()) for n in r[torch.float64][4][i])


FLOOR_ROWS = 512


@functools.lru_cache(maxsize=None)
def same_case_floor(stack, shape, k, b, draws=4):
    """A larger sample of the restatement's own fp32-vs-fp64 noise for a case whose own tensors are too few entries to
    show it (B = 1 and 63 at K = 33, and the deep run), taken from the SAME layers (helpers.parity's noise_floor):
      per sample quantities (z', log_q, d z): FLOOR_ROWS further rows z ~ N(0, 1) with cotangents ~ N(0, 1) through the
        case's own parameters, rows near a kink left out as everywhere; a row's results do not depend on the batch;
      parameter gradients, which are sums over the case's own batch: the case's fp32 gradients taken again with the
        features in ``draws`` other orders - the same arithmetic, other summation orders - every entry keeping the draw
        farthest from the fp64 result (at D = 1 there is one order and this adds nothing).
    The reason for the second: single samples (1 + s h' near 0) can carry a gradient entry, and the restatement's own
    fp32 run in another feature order is then outside parity's bound around its first order: for the 200 tanh layers at
    B = 65 up to 1.8x (4 of 6 orders tried on the CPU), where the kernel was 1.1x outside at d w of layer 198.  What it
    gives, measured on the CPU over the parameter gradients of a case: the five draws' noise is in the median 1.0 to 2.3x
    the single order's and at the 90th percentile up to 6x (deep tanh run 2.3x / 4.9x, deep radial run 1.1x / 4.5x, mixed
    D = 64 B = 1 1.2x / 6.1x, B = 63 1.7x / 5.9x); single entries whose own draw happens to be nearly exact get more
    (74x at d b of layer 198 of the deep tanh run, whose single draw is 4.7e-6).  The further rows give 1 to 6x the
    noise of the case's own rows at B = 63 and 65; at B = 1 the own row is D entries and they give z' 2 to 5x and d z 10
    to 30x of it, more at D = 1 where it is one entry (d z 290x of an own draw of 4e-9).
    Returns {"z", "log_q", "d z": noise, "grads": [per layer {name: noise}]}.  Shared between tests: do not modify."""
    r = reference(stack, shape, k, b)
    r64 = r[torch.float64]
    g = torch.Generator().manual_seed(ref.seed_of("floor", stack, shape, k, b))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    z, g_z, g_ld = rn(FLOOR_ROWS, *tup(shape)), rn(FLOOR_ROWS, *tup(shape)), rn(FLOOR_ROWS)
    with torch.no_grad():
        keep = ~ref.kink_rows(ref.forward(z, r["layers"])[2], r["layers"])
    assert int((~keep).sum()) <= 0.02 * FLOOR_ROWS
    g_z[~keep] = 0
    g_ld[~keep] = 0
    rows = {t: ref.gradients(r["layers"], z, g_z, g_ld, t) for t in DTYPES}
    rows = {t: (rows[t][0], ref.gaussian_log_prob(z.to(t)) - rows[t][1], rows[t][3]) for t in DTYPES}
    per_sample = [float((rows[torch.float32][j].double() - rows[torch.float64][j])[keep].abs().max()) for j in range(3)]

    d = r["z"][0].numel()
    far = lambda x, want: float((x.double() - want).abs().max())
    noise = {"z": per_sample[0], "log_q": per_sample[1], "d z": max(per_sample[2], far(r[torch.float32][3], r64[3])),
             "grads": [{n: far(r[torch.float32][4][i][n], r64[4][i][n]) for n in r64[4][i]} for i in range(k)]}
    for _ in range(draws if d > 1 else 0):
        perm = torch.randperm(d, generator=g)
        back = torch.argsort(perm)
        layers = [{n: (v.reshape(1, d)[:, perm] if n in ("u", "w", "z_0") else v) for n, v in p.items()} for p in r["layers"]]
        res = ref.gradients(layers, r["z"].reshape(b, d)[:, perm], r["g_z"].reshape(b, d)[:, perm], r["g_ld"], torch.float32)
        noise["d z"] = max(noise["d z"], far(res[3][:, back].reshape(r64[3].shape), r64[3]))
        for i, layer in enumerate(res[4]):
            for n, v in layer.items():
                v = v[:, back].reshape(r64[4][i][n].shape) if n in ("u", "w", "z_0") else v
                noise["grads"][i][n] = max(noise["grads"][i][n], far(v, r64[4][i][n]))
    return noise


def needs_floor(k, b):
    return k >= 33 and b < 1000


def run_gradients(model, r, dtype, with_gz=True, with_gld=True):
    """Gradients of (z' g_z).sum() + (log_det g_ld).sum() through the run: (d z, [per layer {name: grad}])."""
    for p in model.parameters():
        p.grad = None
    z = r["z"].to(dtype).cuda().requires_grad_(True)
    out, ld = fused_planar.run(list(model.flows), z, False, None, 1.0)
    loss = 0
    if with_gz:
        loss = loss + (out * r["g_z"].to(dtype).cuda()).sum()
    if with_gld:
        loss = loss + (ld * r["g_ld"].to(dtype).cuda()).sum()
    loss.backward()
    return z.grad, [{n: p.grad.clone() for n, p in f.named_parameters()} for f in model.flows]


def check_gradients(stack, shape, k, b, dtype, floor=None):
    r = reference(stack, shape, k, b)
    model = model_of(r["layers"], shape, dtype)
    tag = "%s %s K=%d B=%d %s" % (stack, shape, k, b, dtype)
    gz, gp = run_gradients(model, r, dtype)
    gz2, gp2 = run_gradients(model, r, dtype)
    assert torch.equal(gz, gz2), tag + ": two backward calls differ"
    pairs = [("d z", gz, r[torch.float32][3], r[torch.float64][3], floor["d z"] if floor else 0.0)]
    for i, layer in enumerate(gp):
        for n, g in layer.items():
            assert torch.equal(g, gp2[i][n]), tag + ": two backward calls differ"
            nfl = layer_noise(r, i) if g.numel() == 1 else 0.0
            if floor:
                nfl = max(nfl, floor["grads"][i][n], max(floor["grads"][i].values()) if g.numel() == 1 else 0.0)
            pairs.append(("d %s of layer %d" % (n, i), g, r[torch.float32][4][i][n], r[torch.float64][4][i][n], nfl))
    for name, got, r32, r64, nfl in pairs:
        got = got.detach().cpu()
        assert got.shape == r64.shape, (tag, name)
        if dtype == torch.float32:
            parity(got, r32, r64, what="%s %s" % (tag, name), noise_floor=nfl or 0.0)
        else:
            bound = 1e-9 * float(r64.abs().max())
            assert float((got - r64).abs().max()) <= bound, "%s %s: %.3e > %.3e" % (tag, name, float((got - r64).abs().max()), bound)


@pytest.mark.parametrize("stack", STACKS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradients(hip, shape, stack):
    for dtype in DTYPES:
        for k, b in RUNS:
            check_gradients(stack, shape, k, b, dtype, floor=same_case_floor(stack, shape, k, b) if needs_floor(k, b) else None)


@pytest.mark.parametrize("stack", ["tanh", "radial"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_gradients_deep_run(hip, stack, dtype):
    k, d, b = DEEP
    check_gradients(stack, d, k, b, dtype, floor=same_case_floor(stack, d, k, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_gradients_with_one_cotangent(hip, dtype):
    stack, shape, k, b = "mixed", 17, 33, 63
    r = reference(stack, shape, k, b)
    layers, z = r["layers"], r["z"]
    model = model_of(layers, shape, dtype)
    for with_gz, with_gld in ((True, False), (False, True)):
        want = {d: ref.gradients(layers, z, r["g_z"] if with_gz else None, r["g_ld"] if with_gld else None, d) for d in DTYPES}
        gz, gp = run_gradients(model, r, dtype, with_gz, with_gld)
        pairs = [(gz, want[torch.float32][3], want[torch.float64][3], 0.0)]
        pairs += [(g, want[torch.float32][4][i][n], want[torch.float64][4][i][n], layer_noise(want, i) if g.numel() == 1 else 0.0)
                  for i, layer in enumerate(gp) for n, g in layer.items()]
        for got, r32, r64, nfl in pairs:
            if dtype == torch.float32:
                parity(got, r32, r64, what="one cotangent", noise_floor=nfl)
            else:
                assert float((got.cpu() - r64).abs().max()) <= 1e-9 * float(r64.abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("kind,d,k", [("tanh", 2, 8), ("radial", 2, 8), ("tanh", 17, 4), ("radial", 17, 4)])
def test_reverse_kld_trains(hip, kind, d, k, dtype):
    """The loss at a given base draw equals the restatement's; backward reaches every parameter; Adam moves them all."""
    torch.manual_seed(31)
    layers, eps, _, _ = ref.inputs(kind, d, k, 256)
    model = model_of(layers, d, dtype)
    target = nf.distributions.DiagGaussian(d, trainable=False)
    target.loc.copy_(torch.linspace(-1.0, 1.0, d).reshape(1, d))
    target.log_scale.fill_(0.3)
    loc, log_scale = target.loc.detach().clone(), target.log_scale.detach().clone()      # .cuda() moves the module itself
    model.p = target.to(dtype).cuda()
    want = {}
    for t in DTYPES:
        z, lq = ref.sample_from(eps.to(t), ref.cast(layers, t))
        want[t] = ((lq.mean() - ref.gaussian_log_prob(z, loc.to(t), log_scale.to(t)).mean()).reshape(1),)
        assert torch.isfinite(want[t][0]).all()
    z, lq = model.sample_from(eps.to(dtype).cuda())
    loss = torch.mean(lq) - torch.mean(model.p.log_prob(z))
    judge(loss.reshape(1), want, dtype, lambda t: t[0], "reverse KLD at a given draw")
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    loss = model.reverse_kld(256)
    assert torch.isfinite(loss)
    loss.backward()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()), n
    opt.step()
    for n, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n + " did not move"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("d,k", [(2, 8), (17, 4)])
def test_forward_kld_trains(hip, d, k, dtype):
    layers, x, _, _ = ref.inputs("leaky_relu", d, k, 256)
    model = model_of(layers, d, dtype)
    want = {}
    for t in DTYPES:
        z, ld = ref.inverse(x.to(t), ref.cast(layers, t))
        want[t] = (-(ref.gaussian_log_prob(z) + ld).mean().reshape(1),)
        assert torch.isfinite(want[t][0]).all()
    loss = model.forward_kld(x.to(dtype).cuda())
    judge(loss.reshape(1), want, dtype, lambda t: t[0], "forward KLD")
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    loss.backward()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and bool((p.grad != 0).any()), n
    opt.step()
    for n, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n + " did not move"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_feature_limit(hip, dtype):
    """At the limit the kernel runs, one feature beyond it the layers take the torch composition: same bounds."""
    limit = 256
    assert nf.lib().vcnf_planar_radial_supported(limit) == 1 and nf.lib().vcnf_planar_radial_supported(limit + 1) == 0
    for d in (limit, limit + 1):
        r = reference("mixed", d, 3, 65)
        model = model_of(r["layers"], d, dtype)
        eps = r["z"].to(dtype).cuda()
        assert (fused_planar.plan(list(model.flows), 0, eps, False) is not None) == (d == limit)
        assert all(fused_planar.covers(f, eps) == (d == limit) for f in model.flows)
        with torch.no_grad():
            z, lq = model.sample_from(eps)
        lq_ref = {t: (log_q_of(r, t),) for t in DTYPES}
        judge(z, r, dtype, lambda t: t[0], "D=%d z" % d, r["keep"])
        judge(lq, lq_ref, dtype, lambda t: t[0], "D=%d log_q" % d, r["keep"])
        if d == limit:
            check_gradients("mixed", d, 3, 65, dtype)


def test_state_dict_round_trip_and_double(hip):
    torch.manual_seed(7)
    make = lambda: nf.NormalizingFlow(nf.distributions.DiagGaussian(5), [Planar(5), Radial(5), Planar(5, act="leaky_relu")])
    a, b = make().cuda(), make().cuda()
    b.load_state_dict(a.state_dict())
    eps = torch.randn(33, 5, device="cuda")
    with torch.no_grad():
        za, qa = a.sample_from(eps)
        zb, qb = b.sample_from(eps)
        assert torch.equal(za, zb) and torch.equal(qa, qb)
        a.double()
        assert all(p.dtype == torch.float64 for p in a.parameters()) and a.flows[1].d.dtype == torch.int64
        zd, qd = a.sample_from(eps.double())
    assert zd.dtype == torch.float64 and torch.allclose(zd.float(), za, rtol=1e-4, atol=1e-4) and torch.allclose(qd.float(), qa, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
def test_mixed_model_plans_the_other_families_as_before(hip, dtype, monkeypatch):
    """A Planar / Radial run between runs of MaskedAffineFlow + ActNorm layers: each family's planner takes its own
    stretch, and sample_from matches the layer-by-layer walk."""
    from vcnf_amd import fused_masked
    torch.manual_seed(11)
    d = 4
    mask = torch.tensor([1.0 if i % 2 == 0 else 0.0 for i in range(d)])

    def pair(i):
        s, t = nf.nets.MLP([d, 8, d], init_zeros=True), nf.nets.MLP([d, 8, d], init_zeros=True)
        return [nf.flows.MaskedAffineFlow(mask if i % 2 == 0 else 1 - mask, t, s), nf.flows.ActNorm(d)]
    flows = pair(0) + pair(1) + [Planar(d), Radial(d), Planar(d, act="leaky_relu")] + pair(2) + pair(3)
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(d), flows)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".net.2." in n:
                p.normal_(0.0, 0.1)
    model = model.to(dtype).cuda().eval()
    eps = torch.randn(257, d, device="cuda", dtype=dtype)
    calls = []
    for mod, name in ((fused_masked, "masked"), (fused_planar, "planar")):
        real = mod.run
        monkeypatch.setattr(mod, "run", lambda steps, *a, _real=real, _name=name: (calls.append((_name, len(steps))), _real(steps, *a))[1])
    with torch.no_grad():
        model.fuse_masked_stacks = model.fuse_planar_stacks = False
        model.sample_from(eps)                               # the first batch initialises the ActNorm layers
        want = model.sample_from(eps)
        calls.clear()
        model.fuse_masked_stacks = model.fuse_planar_stacks = True
        got = model.sample_from(eps)
    assert calls == [("masked", 4), ("planar", 3), ("masked", 4)]
    tol = dict(rtol=2e-5, atol=2e-5) if dtype == torch.float32 else dict(rtol=1e-11, atol=1e-11)
    for a, b in zip(got, want):
        assert torch.isfinite(b).all() and torch.allclose(a, b, **tol), float((a - b).abs().max())


def test_subclasses_take_the_torch_composition(hip):
    """What a subclass overrides is unknown to the kernel path: it joins no run and evaluates its own composition."""
    class MyPlanar(Planar):
        pass

    class MyRadial(Radial):
        pass
    r = reference("mixed", 5, 3, 65)
    z = r["z"].cuda()
    for p in r["layers"]:
        base = module_of(p, 5, torch.float64).cuda()
        sub = (MyRadial if p["kind"] == "radial" else MyPlanar).__new__(MyRadial if p["kind"] == "radial" else MyPlanar)
        sub.__dict__.update(base.__dict__)
        assert fused_planar.covers(base, z) and not fused_planar.covers(sub, z)
        assert fused_planar.plan([sub, base], 0, z, False) is None and fused_planar.plan([base, sub], 0, z, False)[0] == 1
        with torch.no_grad():
            got, want = sub(z), base(z)
        assert_close(got[0], want[0], what="subclass z", **F64)
        assert_close(got[1], want[1], what="subclass log_det", **F64)
