"""The stochastic layers on the GPU (csrc/stochastic.hip through vcnf_amd._lib, vcnf_amd.autograd, the modules and
NormalizingFlow) against the plain-torch restatement stochastic_ref.py run on the CPU with the same draws.

Decisions must be the fp64 restatement's on every row outside the near-tie band (|min(prob, 2) - unif| < 1e-2 for HMC,
|min(exp(.), 1) - w| < 1e-3 at any step for MH); rows inside it are left out of the value comparisons, and the share of a
case's decisions in the band is asserted under 2 % (test_stochastic_abi.py pins both on the CPU).  fp32 values are judged
by helpers.parity against the restatement's fp32 and fp64 runs, with the noise of the B = 1000 case of the same
configuration as noise_floor for the smaller batches.  fp64 values are judged against the fp64 restatement with a
yardstick of its own: the restatement evaluated with autograd scores and with the closed-form scores of
include/vcnf_hip.h - the same mathematics, other roundings - differs by at most 1.8e-12 in z_out and 1.2e-10 in log_det
over the cases here at B = 1000 (1.2e-12 and 2.5e-11 over their three-layer runs), and the tolerance is 16 times that
difference for the case plus 1e-12 of the largest entry; the factor covers the kernel's exp / log being another
library's.  Gradients follow the same two rules, against autograd of the restatement with the kernel's own decisions
imposed, so that a band row cannot become a gradient mismatch.

Measured on an MI355X: the fp64 kernels are within 1.8e-12 (z_out), 1.3e-10 (log_det), 8.5e-10 (g_z) and 2.2e-9 (parameter
gradients of size 1e3 - 4e5) of the fp64 restatement; the fp32 kernels' largest errors against it are 5.6e-4, 1.9e-2, 0.74
and 0.80 where the fp32 restatement's own are 1.4e-3, 5.5e-2, 0.48 and 0.84; the MH rows are the fp64 restatement's bit
for bit; log_det with unif = 0 is the target kernel's log p(z) - log p(z_out) bit for bit in both precisions."""
import pytest
import torch

import stochastic_ref as sref
import target_ref as ref
import vcnf_amd as nf
from helpers import parity
from vcnf_amd import _lib, fused_stochastic

pytestmark = pytest.mark.gpu

DTYPES = list(sref.DTYPES)
IDS = ["fp32", "fp64"]
case_id = lambda c: "-".join(str(x) for x in c) if isinstance(c, tuple) else str(c)


def target_of(family, n, dtype):
    D = nf.distributions
    t = D.TwoMoons() if family == "two_moons" else D.CircularGaussianMixture(n) if family == "circular" else D.RingMixture(n)
    return (t.double() if dtype == torch.float64 else t).cuda()


def layers_of(target, params, steps, dtype):
    return [nf.flows.HamiltonianMonteCarlo(target, steps, ls.to(dtype), lm.to(dtype)).cuda() for ls, lm in params]


def hmc_kernel(target, layers, z, noise, unif, steps, want_trace=True):
    table, scale = target._operands(z)
    with torch.no_grad():
        step, mass, sqm = fused_stochastic.operands(layers)
        return _lib.hmc_stack(z, noise, unif, step, mass, sqm, steps, target._family, table, scale, want_trace=want_trace)


def fp64_bound(yardstick, want):
    return 16.0 * yardstick + 1e-12 * float(want.abs().max())


def judge(got, r32, r64, dtype, what, noise_floor=0.0, yardstick=0.0):
    """fp32: helpers.parity; fp64: |got - r64| <= 16 yardstick + 1e-12 max|r64|, same NaN pattern."""
    got = got.detach().cpu()
    assert got.dtype == dtype and got.shape == r64.shape, what
    err = float((got.double() - r64).abs().max()) if got.numel() else 0.0
    print("%s: max |got - fp64 restatement| %.3e (the fp32 restatement's %.3e)" % (
        what, err, float((r32.double() - r64).abs().max()) if got.numel() else 0.0))
    if dtype == torch.float32:
        parity(got, r32, r64, what=what, noise_floor=noise_floor)
    else:
        bound = fp64_bound(yardstick, r64)
        assert torch.isfinite(got).all() and err <= bound, "%s: %.3e > %.3e" % (what, err, bound)


def kept(r):
    return ~r["near"]


def hmc_floor(case, k, j):
    """Noise of quantity j (0 z_out, 1 log_det) on the kept rows of the B = 1000 case with K = 1."""
    big = sref.hmc_reference(*case, 1000, 1)
    keep = kept(big)
    return float((big[torch.float32][j].double() - big[torch.float64][j])[keep].abs().max())


# ---------------------------------------------------------------- HMC forward
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", sref.HMC_CASES, ids=case_id)
def test_hmc_forward(hip, case, dtype):
    family, n, steps, step = case
    target = target_of(family, n, dtype)
    assert sref.hmc_band_share(*case) <= sref.BAND_CAP
    for b, k in [(b, 1) for b in sref.BATCHES] + [(1000, sref.RUN)]:
        r = sref.hmc_reference(*case, b, k)
        tag = "%s B=%d K=%d %s" % (case_id(case), b, k, IDS[DTYPES.index(dtype)])
        layers = layers_of(target, r["params"], steps, dtype)
        z, noise, unif = (r[name].to(dtype).cuda() for name in ("z", "noise", "unif"))
        out, ld, trace, accept = hmc_kernel(target, layers, z, noise, unif, steps)
        again = hmc_kernel(target, layers, z, noise, unif, steps)
        plain = hmc_kernel(target, layers, z, noise, unif, steps, want_trace=False)
        assert all(torch.equal(x, y) for x, y in zip((out, ld, trace, accept), again)), tag + ": two calls differ"
        assert torch.equal(out, plain[0]) and torch.equal(ld, plain[1]), tag + ": the run depends on whether the trace is written"
        assert accept.dtype == torch.uint8 and tuple(accept.shape) == (k, b) and tuple(trace.shape) == (k, b, 2)
        assert torch.equal(trace[0], z) and int(accept.max()) <= 1
        keep = kept(r)
        assert sref.few_near(r["near"], k), "%s: %d rows in the band" % (tag, int(r["near"].sum()))
        differ = (accept.bool().cpu() != r[torch.float64][2]).any(0) & keep
        assert not differ.any(), "%s: %d rows outside the band decided differently" % (tag, int(differ.sum()))
        floors = (0.0, 0.0) if b == 1000 else (hmc_floor(case, k, 0), hmc_floor(case, k, 1))
        yard = sref.hmc_reference(*case, 1000, k)["yardstick"]
        for j, (name, got) in enumerate((("z_out", out), ("log_det", ld))):
            judge(got.cpu()[keep], r[torch.float32][j][keep], r[torch.float64][j][keep], dtype, "%s %s" % (tag, name), floors[j], yard[j])
        # a rejected row is z bit for bit, and its log_det 0; the layers of a run hand their rows on
        for layer in range(k):
            rejected = ~accept[layer].bool()
            after = trace[layer + 1] if layer + 1 < k else out
            assert torch.equal(after[rejected], trace[layer][rejected]), tag
        if k == 1:
            assert not ld[~accept[0].bool()].any(), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", sref.DEFAULTS, ids=case_id)
def test_hmc_unusual_rows(hip, tgt, dtype):
    family, n = tgt
    steps, step, b = 8, 0.1, 65
    target = target_of(family, n, dtype)
    r = sref.hmc_reference(family, n, steps, step, b, 1)
    layers = layers_of(target, r["params"], steps, dtype)
    z, noise, unif = (r[name].to(dtype).cuda() for name in ("z", "noise", "unif"))
    out, ld, trace, accept = hmc_kernel(target, layers, z, noise, unif, steps)
    # unif = 0: every row whose probability is not 0 is accepted, and log_det is the module's own log p(z) - log p(z_out)
    out0, ld0, _, accept0 = hmc_kernel(target, layers, z, noise, torch.zeros_like(unif), steps)
    positive = r[torch.float64][3][0] > 1e-30
    assert bool(accept0[0].bool().cpu()[positive].all()) and int(positive.sum()) > b // 2
    with torch.no_grad():
        lp, lp_out = target.log_prob(z), target.log_prob(out0)
    eps = torch.finfo(dtype).eps
    bound = 4 * eps * torch.maximum(lp.abs(), lp_out.abs()) + 4 * eps
    err = (ld0 - (lp - lp_out)).abs()
    print("%s %s: log_det against the target's kernel, max error %.3e, %d of %d rows bitwise" % (
        case_id(tgt), dtype, float(err.max()), int((ld0 == lp - lp_out).sum()), b))
    assert bool((err <= bound).all())
    # steps = 0: z and zeros, whatever the draws
    same, zeros, _, acc = hmc_kernel(target, layers_of(target, r["params"], 0, dtype), z, noise, unif, 0)
    assert torch.equal(same, z) and not zeros.any() and bool(acc.bool().all())
    # a NaN row: NaN log_det, the row unchanged, the others as they were
    zn, nn_, un = ref.nan_row(z), torch.cat([noise, noise[:, :1]], 1), torch.cat([unif, unif[:, :1]], 1)
    outn, ldn, _, accn = hmc_kernel(target, layers, zn, nn_, un, steps)
    assert torch.equal(outn[:-1], out) and torch.equal(ldn[:-1], ld) and torch.equal(accn[:, :-1], accept)
    assert bool(torch.isnan(ldn[-1])) and bool(torch.isnan(outn[-1, 0])) and float(outn[-1, 1]) == 1.0 and int(accn[0, -1]) == 0
    # element accesses: z one element past its allocation's alignment gives the bits of the aligned call
    buf = torch.empty(2 * b + 1, dtype=dtype, device="cuda")
    buf[1:] = z.reshape(-1)
    shifted = buf[1:].view(b, 2)
    assert shifted.data_ptr() % (2 * z.element_size()) == z.element_size()
    outs, lds, _, accs = hmc_kernel(target, layers, shifted, noise, unif, steps)
    assert torch.equal(outs, out) and torch.equal(lds, ld) and torch.equal(accs, accept)
    # likewise the VJP (its trace one element off) and the Metropolis-Hastings walk (its z), on the draws at hand
    buf[1:] = trace.reshape(-1)
    table, scale = target._operands(z)
    with torch.no_grad():
        step_, mass, sqm = fused_stochastic.operands(layers)
        vjp = lambda t: _lib.hmc_stack_bwd(t, accept, noise, step_, mass, sqm, steps, target._family, table, scale, g_out=noise[0], g_ld=unif[0])
        assert all(torch.equal(x, y) for x, y in zip(vjp(buf[1:].view(1, b, 2)), vjp(trace)))
        buf[1:] = z.reshape(-1)
        walk = lambda x: _lib.mh_walk(x, noise, unif, step_[0], target._family, table, scale, want_accept=True)
        assert all(torch.equal(x, y) for x, y in zip(walk(shifted), walk(z)))


def test_bad_inputs_raise(hip):
    target = target_of("circular", 8, torch.float32)
    f = lambda *shape, dtype=torch.float32: torch.ones(*shape, dtype=dtype, device="cuda")
    z = f(4, 2)
    table, scale = target._operands(z)
    good = dict(z=z, noise=f(1, 4, 2), unif=f(1, 4), step=f(1, 2), mass=f(1, 2), sqrt_mass=f(1, 2))
    call = lambda steps=2, table=table, **kw: _lib.hmc_stack(*{**good, **kw}.values(), steps, target._family, table, scale)
    assert tuple(call()[0].shape) == (4, 2)
    for bad in (dict(z=f(4, 3)), dict(z=f(4)), dict(z=f(4, 2, dtype=torch.float16)), dict(z=torch.ones(4, 2)), dict(noise=f(1, 4, 3)),
                dict(noise=f(2, 4, 2)), dict(unif=f(1, 5)), dict(unif=f(1, 4, dtype=torch.float64)), dict(step=f(2)), dict(mass=f(2, 2)),
                dict(sqrt_mass=torch.ones(1, 2)), dict(steps=-1), dict(table=None), dict(table=table.double()),
                dict(steps=1 << 16)):                                  # the entry point's limit on n_layers (steps + 1)
        with pytest.raises(nf.VcnfError):
            call(**bad)
    with pytest.raises(nf.VcnfError):
        _lib.mh_walk(z, f(2, 4, 2), f(2, 5), f(2), target._family, table, scale)
    with pytest.raises(nf.VcnfError):
        _lib.mh_walk(z, f(2, 4, 2), f(2, 4), f(3), target._family, table, scale)
    with pytest.raises(nf.VcnfError):
        _lib.hmc_stack_bwd(f(1, 4, 2), f(1, 4), f(1, 4, 2), f(1, 2), f(1, 2), f(1, 2), 2, target._family, table, scale)   # accept: not bytes
    empty = dict(z=f(0, 2), noise=f(1, 0, 2), unif=f(1, 0))
    out, ld = call(**empty)
    assert tuple(out.shape) == (0, 2) and tuple(ld.shape) == (0,)
    assert tuple(_lib.mh_walk(f(0, 2), f(3, 0, 2), f(3, 0), f(2), target._family, table, scale).shape) == (0, 2)


# ---------------------------------------------------------------- HMC gradients
def restatement_gradients(case, r, k, accept, gz, gl, dtype, numel=2, score=ref.score):
    """(g_z, [g_log_step_size, g_log_mass per layer ...]) by autograd of the restatement in ``dtype`` on the CPU."""
    family, n, steps, step = case
    z = r["z"].to(dtype).clone().requires_grad_(True)
    params = [(ls[:numel].to(dtype).clone().requires_grad_(True), lm[:numel].to(dtype).clone().requires_grad_(True))
              for ls, lm in r["params"]]
    out, ld, _, _ = sref.hmc_run(family, n, z, r["noise"].to(dtype), r["unif"].to(dtype), params, steps, score=score, accept=accept)
    leaves = [z] + [t for pair in params for t in pair]
    return torch.autograd.grad((out * gz.to(dtype)).sum() + (ld * gl.to(dtype)).sum(), leaves)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", sref.HMC_CASES, ids=case_id)
def test_hmc_gradients(hip, case, dtype):
    """g_z, g_log_step_size and g_log_mass of a three-layer run at B = 1000 and of one layer at B = 65, with parameters of
    two elements and of one."""
    family, n, steps, step = case
    target = target_of(family, n, dtype)
    for b, k, numel in ((1000, sref.RUN, 2), (65, 1, 2), (65, 1, 1)):
        r = sref.hmc_reference(*case, b, k)
        tag = "%s B=%d K=%d numel=%d %s" % (case_id(case), b, k, numel, IDS[DTYPES.index(dtype)])
        g = torch.Generator().manual_seed(ref.seed_of("cotangent", case, b))
        gz, gl = torch.randn(b, 2, generator=g, dtype=torch.float64), torch.randn(b, generator=g, dtype=torch.float64)
        layers = layers_of(target, [(ls[:numel], lm[:numel]) for ls, lm in r["params"]], steps, dtype)
        z, noise, unif = (r[name].to(dtype).cuda() for name in ("z", "noise", "unif"))
        table, scale = target._operands(z)
        runs = []
        for _ in range(2):
            x = z.clone().requires_grad_(True)
            for layer in layers:
                layer.zero_grad(set_to_none=True)
            step_, mass, sqm = fused_stochastic.operands(layers)
            out, ld = nf.autograd.HmcStackFn.apply(x, step_, mass, sqm, noise, unif, steps, target._family, table, scale)
            assert type(out.grad_fn).__name__.startswith("HmcStackFn")                           # ONE node
            ((out * gz.to(dtype).cuda()).sum() + (ld * gl.to(dtype).cuda()).sum()).backward()
            runs.append([x.grad.clone()] + [p.grad.clone() for layer in layers for p in (layer.log_step_size, layer.log_mass)])
        assert all(torch.equal(a, c) for a, c in zip(*runs)), tag + ": two backward calls differ"
        accept = hmc_kernel(target, layers, z, noise, unif, steps)[3].bool().cpu()
        want32 = restatement_gradients(case, r, k, accept, gz, gl, torch.float32, numel)
        want64 = restatement_gradients(case, r, k, accept, gz, gl, torch.float64, numel)
        closed = restatement_gradients(case, r, k, accept, gz, gl, torch.float64, numel, score=sref.closed_form_score)
        names = ["g_z"] + ["g_%s[%d]" % (p, i) for i in range(k) for p in ("log_step_size", "log_mass")]
        for name, got, w32, w64, c64 in zip(names, runs[0], want32, want64, closed):
            assert tuple(got.shape) == tuple(w64.shape) and bool((got != 0).any()), "%s %s" % (tag, name)
            judge(got, w32, w64, dtype, "%s %s" % (tag, name), yardstick=float((c64 - w64).abs().max()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", sref.DEFAULTS, ids=case_id)
def test_hmc_gradients_with_rejected_non_finite_rows(hip, tgt, dtype):
    """Rows that cannot be accepted - a NaN row, an inf row, and a finite row whose leapfrog runs far off, in fp32 to inf / NaN (a
    momentum draw of 1e30) - appended to a three-layer run at B = 1000: they are rejected in every layer, the parameter
    gradients are finite and have the bits of the run without them (the appended rows fall into a workgroup of their
    own lanes' zeros: 1000 + 3 rows are the same four tiles, and exact zeros change no sum), g_z of the other rows is
    unchanged, and the appended rows hand their gz through."""
    family, n = tgt
    case = (family, n, 8, 0.1)
    steps, k, b = 8, sref.RUN, 1000
    target = target_of(family, n, dtype)
    r = sref.hmc_reference(*case, b, k)
    layers = layers_of(target, r["params"], steps, dtype)
    z, noise, unif = (r[name].to(dtype).cuda() for name in ("z", "noise", "unif"))
    extra_z = torch.tensor([[float("nan"), 1.0], [float("inf"), 0.5], [0.3, -0.4]], dtype=dtype, device="cuda")
    extra_noise = noise[:, :3].clone()
    extra_noise[:, 2] = 1e30
    g = torch.Generator().manual_seed(ref.seed_of("cotangent-nan", tgt))
    gz = torch.randn(b + 3, 2, generator=g, dtype=torch.float64).to(dtype).cuda()
    gl = torch.randn(b + 3, generator=g, dtype=torch.float64).to(dtype).cuda()
    table, scale = target._operands(z)

    def gradients(z, noise, unif, gz, gl):
        x = z.clone().requires_grad_(True)
        for layer in layers:
            layer.zero_grad(set_to_none=True)
        step, mass, sqm = fused_stochastic.operands(layers)
        out, ld = nf.autograd.HmcStackFn.apply(x, step, mass, sqm, noise, unif, steps, target._family, table, scale)
        # the appended rows' own z_out and log_det are not finite: the loss takes them through their cotangents alone
        torch.autograd.backward((out, ld), (gz, gl))
        return x.grad, [p.grad.clone() for layer in layers for p in (layer.log_step_size, layer.log_mass)]

    gx, gp = gradients(z, noise, unif, gz[:b], gl[:b])
    gx3, gp3 = gradients(torch.cat([z, extra_z]), torch.cat([noise, extra_noise], 1), torch.cat([unif, unif[:, :3]], 1), gz, gl)
    accept = hmc_kernel(target, layers, torch.cat([z, extra_z]), torch.cat([noise, extra_noise], 1), torch.cat([unif, unif[:, :3]], 1), steps)[3]
    assert not accept[:, b:].any() and bool(accept[:, :b].any())
    for a, c in zip(gp, gp3):
        assert torch.isfinite(c).all() and bool((c != 0).any()) and torch.equal(a, c), (a.tolist(), c.tolist())
    assert torch.equal(gx3[:b], gx) and torch.isfinite(gx).all()
    assert torch.equal(gx3[b:], gz[b:])


# ---------------------------------------------------------------- MH
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", sref.TARGETS, ids=case_id)
def test_mh_walk(hip, tgt, dtype):
    family, n = tgt
    target = target_of(family, n, dtype)
    for steps in sref.MH_STEPS:
        for scale in sref.MH_SCALES:
            assert sref.mh_band_share(family, n, steps, scale) <= sref.BAND_CAP
            big = sref.mh_reference(family, n, steps, scale, 1000)
            floor = float((big[torch.float32][0].double() - big[torch.float64][0])[kept(big)].abs().max())
            for b in sref.MH_BATCHES:
                r = sref.mh_reference(family, n, steps, scale, b)
                tag = "%s steps %d scale %s B=%d %s" % (case_id(tgt), steps, scale, b, IDS[DTYPES.index(dtype)])
                z, eps, w = (r[name].to(dtype).cuda() for name in ("z", "eps", "w"))
                prop = torch.tensor(scale, dtype=dtype, device="cuda")
                table, tscale = target._operands(z)
                out, accept = _lib.mh_walk(z, eps, w, prop, target._family, table, tscale, want_accept=True)
                assert torch.equal(out, _lib.mh_walk(z, eps, w, prop, target._family, table, tscale)), tag
                keep = kept(r)
                assert sref.few_near(r["near"]), "%s: %d rows in the band" % (tag, int(r["near"].sum()))
                differ = (accept.bool().cpu() != r[torch.float64][2]).any(0) & keep
                assert not differ.any(), "%s: %d rows outside the band decided differently" % (tag, int(differ.sum()))
                judge(out.cpu()[keep], r[torch.float32][0][keep], r[torch.float64][0][keep], dtype, tag + " z_out",
                      0.0 if b == 1000 else floor)
                stay = ~accept.bool().any(0)
                assert torch.equal(out[stay], z[stay]), tag
    # the module: the same draws from torch's generator as its torch path, log_det exactly zero, the identity backwards
    prop = nf.distributions.DiagGaussianProposal((2,), [0.3, 0.24]).to(dtype).cuda()
    layer = nf.flows.MetropolisHastings(target, prop, 4)
    plain = nf.flows.MetropolisHastings(sref.plain_target(family, n).cuda(), prop, 4)
    z = sref.inputs(family, n, 1000).to(dtype).cuda()
    assert fused_stochastic.covers_walk(layer, z) and not fused_stochastic.covers_walk(plain, z)
    # a walk longer than one launch takes is the torch composition's, not an error
    assert not fused_stochastic.covers_walk(nf.flows.MetropolisHastings(target, prop, fused_stochastic.MAX_POINTS), z)
    assert fused_stochastic.covers_walk(nf.flows.MetropolisHastings(target, prop, fused_stochastic.MAX_POINTS - 1), z)
    torch.manual_seed(29)
    x = z.clone().requires_grad_(True)
    out, ld = layer(x)
    assert ld.dtype == dtype and tuple(ld.shape) == (1000,) and not ld.any()
    # the module's draws, regenerated as the reference's layer makes them - per step the proposal's randn of [B, 2], then
    # rand of [B] - and given to the kernel: the module's rows bit for bit, which pins the order of its draws
    torch.manual_seed(29)
    eps, w = torch.empty(4, 1000, 2, dtype=dtype, device="cuda"), torch.empty(4, 1000, dtype=dtype, device="cuda")
    for i in range(4):
        eps[i] = torch.randn((1000,) + prop.shape, dtype=dtype, device="cuda")
        w[i] = torch.rand(1000, dtype=dtype, device="cuda")
    table, tscale = target._operands(z)
    assert torch.equal(out.detach(), _lib.mh_walk(z, eps, w, prop.scale[0], target._family, table, tscale)), case_id(tgt)
    # and the torch path under the same seed walks the same chain, up to decisions at near ties
    torch.manual_seed(29)
    want, want_ld = plain(z)
    assert not want_ld.any()
    moved = (out.detach() - want).abs().max(1)[0] > 1e-3                 # another decision somewhere along the walk
    assert float(moved.double().mean()) <= sref.BAND_CAP, "%s: %d rows walk differently on the two paths" % (case_id(tgt), int(moved.sum()))
    gz = torch.randn(1000, 2, dtype=dtype, device="cuda")
    grad, = torch.autograd.grad((out * gz).sum(), x)
    assert torch.equal(grad, gz)
    torch.manual_seed(29)
    with torch.no_grad():
        assert torch.equal(layer.inverse(z)[0], out.detach())            # inverse is forward


# ---------------------------------------------------------------- the model
def model_of(target, dtype, seed=43):
    torch.manual_seed(seed)
    params = sref.hmc_parameters(0.05, sref.RUN)
    flows = [nf.flows.Planar(2, act="leaky_relu") for _ in range(4)] + [nf.flows.HamiltonianMonteCarlo(target, 5, ls.float(), lm.float()) for ls, lm in params]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), flows, p=target)
    return (model.double() if dtype == torch.float64 else model).cuda()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", sref.DEFAULTS, ids=case_id)
def test_model_runs_and_trains(hip, tgt, dtype, monkeypatch):
    family, n = tgt
    target = target_of(family, n, dtype)
    model = model_of(target, dtype)
    assert model.fuse_stochastic_stacks is True
    calls = []
    launch = _lib.hmc_stack
    monkeypatch.setattr(_lib, "hmc_stack", lambda *a, **kw: calls.append(a[3].shape[0]) or launch(*a, **kw))
    results = {}
    for fuse in (True, False):
        model.fuse_stochastic_stacks = fuse
        for name, call in (("sample", lambda: model.sample(1024)),
                           ("log_prob", lambda: (None, model.log_prob(sref.inputs(family, n, 1000).to(dtype).cuda())))):
            del calls[:]
            torch.manual_seed(7)
            with torch.no_grad():
                results[name, fuse] = call()
            assert calls == ([3] if fuse else [1, 1, 1]), "%s fuse=%s: HMC launches %s" % (name, fuse, calls)
    model.fuse_stochastic_stacks = True
    # one launch or three: the same kernel arithmetic layer by layer, so the rows are the same bits; log q adds the three
    # log_dets in another order
    z, log_q = results["sample", True]
    z1, log_q1 = results["sample", False]
    assert z.dtype == dtype and tuple(z.shape) == (1024, 2) and torch.isfinite(z).all()
    assert torch.equal(z, z1), "%d rows differ between one launch and three" % int((z != z1).any(1).sum())
    eps = torch.finfo(dtype).eps
    for a, c in ((log_q, log_q1), (results["log_prob", True][1], results["log_prob", False][1])):
        ok = torch.isfinite(c)
        assert torch.equal(torch.isfinite(a), ok) and bool(((a - c)[ok].abs() <= 64 * eps * (1 + c[ok].abs())).all())
    # one reverse_kld step: the run is one node of the plain walk, and all six HMC parameters get a gradient.  At beta = 1
    # that gradient is zero by the layer's own definition - log_det = log p(z) - log p(z_out) telescopes with the
    # objective's -log p(z_out), so the loss does not depend on where an accepted row lands - and the kernel gives the
    # exact 0, because its score at z_out has the bits of the target's; an annealed step (beta = 0.5) moves every parameter
    hmc = [(k, p) for k, p in model.named_parameters() if "log_" in k and k.startswith("flows.")]
    assert len(hmc) == 6
    for beta in (1.0, 0.5):
        runs = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            del calls[:]
            torch.manual_seed(9)
            loss = model.reverse_kld(512, beta=beta)
            loss.backward()
            assert calls == [3] and loss.dtype == dtype and bool(torch.isfinite(loss))
            runs.append([p.grad.clone() for p in model.parameters()])
        for k, p in hmc:
            assert torch.isfinite(p.grad).all(), k
            assert bool((p.grad != 0).all()) if beta != 1.0 else not p.grad.any(), "%s at beta = %g: %s" % (k, beta, p.grad.tolist())
        assert all(torch.isfinite(g).all() for g in runs[0]) and all(torch.equal(a, c) for a, c in zip(*runs))


@pytest.mark.parametrize("tgt", sref.DEFAULTS, ids=case_id)
def test_other_targets_take_the_torch_path(hip, tgt):
    """A Target subclass that is none of the kernel targets runs the reference's composition on the device (fp64) and
    matches the restatement on the CPU with the same draws: decisions outside the band, values to 1e-9 of the largest
    entry (device and host libraries round exp, log and the norm differently, and eight leapfrog steps carry that on)."""
    family, n = tgt
    steps, step, b = 8, 0.1, 1000
    ls, lm = sref.hmc_parameters(step)[0]
    layer = nf.flows.HamiltonianMonteCarlo(sref.plain_target(family, n), steps, ls.clone(), lm.clone()).cuda()
    z = sref.inputs(family, n, b).cuda()
    assert not fused_stochastic.covers(layer, z)
    torch.manual_seed(31)
    with torch.no_grad():
        out, ld = layer(z)
    torch.manual_seed(31)
    noise = torch.randn_like(z)
    unif = torch.rand(b, dtype=z.dtype, device="cuda")
    want, want_ld, accept, prob = sref.hmc_layer(family, n, z.cpu(), noise.cpu(), unif.cpu(), ls, lm, steps)
    keep = ~((torch.clamp(prob, max=2.0) - unif.cpu()).abs() < sref.HMC_BAND)
    assert float((~keep).double().mean()) <= sref.BAND_CAP
    for name, got, w in (("z_out", out, want), ("log_det", ld, want_ld)):
        err, top = float((got.cpu() - w)[keep].abs().max()), float(w[keep].abs().max())
        print("%s torch path %s: max error %.3e of %.3e" % (case_id(tgt), name, err, top))
        assert err <= 1e-9 * top, name
    # and the kernel target with the same seed walks the same chain outside the band
    kernel = nf.flows.HamiltonianMonteCarlo(target_of(family, n, torch.float64), steps, ls.clone(), lm.clone()).cuda()
    assert fused_stochastic.covers(kernel, z)
    torch.manual_seed(31)
    with torch.no_grad():
        out_k, ld_k = kernel(z)
    err = float((out_k.cpu() - want)[keep].abs().max())
    assert err <= 1e-9 * float(want[keep].abs().max()), "kernel path under the same seed: %.3e" % err
