"""Hamiltonian annealed importance sampling on the GPU (the annealed kernels of csrc/stochastic.hip through vcnf_amd._lib,
vcnf_amd.autograd, nf.sampling.HAIS and NormalizingFlow) against the plain-torch restatement hais_ref.py run on the CPU
with the same draws.

The rules are test_gpu_stochastic.py's.  Decisions must be the fp64 restatement's on every row outside the near-tie
band (|min(prob, 2) - unif| < 1e-2 in any layer); rows inside it are left out of the value comparisons and their share is
pinned on the CPU (test_hais_abi.py).  fp32 values are judged by helpers.parity against the restatement's fp32 and fp64
chains, with the noise of the B = 1000 chain of the same case as noise_floor for the smaller batches.  fp64 values are
judged against 16 times the case's own yardstick - the fp64 restatement with autograd scores against the one with the
closed-form scores of include/vcnf_hip.h - plus 1e-12 of the largest entry.  Gradients follow the same two rules against
autograd of the restatement with the kernel's decisions imposed.

Measured on an MI355X: the fp64 kernels are within 1.2e-11 (z_out), 7.0e-11 (log_det), 5.7e-11 (g_z) and 2.1e-10
(parameter gradients) of the fp64 restatement; the fp32 kernels' largest errors against it are 2.6e-2, 3.0e-2, 5.9e-2 and
0.14 where the fp32 restatement's own are 6.1e-3, 2.7e-2, 6.3e-2 and 0.17 (the case that rejects often sets all of
them).  A run is its layers one by one, beta = 1 is vcnf_hmc_stack_* and logp_target is the target kernel's log p, all
bit for bit; with beta = 0 and unif = 0 log_det is within 1.8e-15 (fp64) and 9.6e-7 (fp32) of the prior kernel's
log p(z) - log p(z_out), where 4 eps of the larger term allows 7e-15 and 3.8e-6.  HAIS.sample(1000) with six betas
estimates log Z within 1e-6 (fp32) of the restatement's.  The file takes 12 s.

One seed of the forward tests was replaced after its first run on the GPU; hais_ref.SALTS says why, with the figures."""
import math

import pytest
import torch

import grid_caps as gc
import hais_ref as href
import stochastic_ref as sref
import target_ref as ref
import vcnf_amd as nf
from test_gpu_stochastic import DTYPES, IDS, case_id, judge, layers_of, target_of
from vcnf_amd import _lib, fused_stochastic

pytestmark = pytest.mark.gpu

M = href.MS[0]


def tag_of(dtype):
    return IDS[DTYPES.index(dtype)]


def prior_operands(dtype):
    return tuple(t.cuda() for t in href.prior_parameters(dtype))


def prior_of(dtype, trainable=False):
    """The restatement's prior as the package's DiagGaussian on the device."""
    prior = nf.distributions.DiagGaussian(2, trainable=trainable)
    prior = (prior.double() if dtype == torch.float64 else prior).cuda()
    loc, log_scale = prior_operands(dtype)              # in the dtype itself: 0.3 is not a float
    with torch.no_grad():
        prior.loc.copy_(loc.reshape(1, 2))
        prior.log_scale.copy_(log_scale.reshape(1, 2))
    return prior


def annealed_kernel(target, layers, z, noise, unif, steps, betas, want_trace=True, want_logp=False):
    table, scale = target._operands(z)
    loc, log_scale = prior_operands(z.dtype)
    with torch.no_grad():
        step, mass, sqm = fused_stochastic.operands(layers)
        return _lib.hmc_annealed_stack(z, noise, unif, step, mass, sqm, betas.to(z.dtype).cuda(), loc, log_scale, steps,
                                       target._family, table, scale, want_trace=want_trace, want_logp=want_logp)


def device_inputs(r, dtype):
    return tuple(r[name].to(dtype).cuda() for name in ("z", "noise", "unif"))


def floor_of(case, j):
    """Noise of quantity j (0 z_out, 1 log_det) on the kept rows of the case's B = 1000 chain at M = 4."""
    big = href.reference(*case, 1000, M)
    return float((big[torch.float32][j].double() - big[torch.float64][j])[~big["near"]].abs().max())


# ---------------------------------------------------------------- 1. forward parity
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", href.CASES, ids=case_id)
def test_forward(hip, case, dtype):
    family, n, steps, step = case
    target = target_of(family, n, dtype)
    assert href.band_share(case) <= sref.BAND_CAP
    for b, m in href.runs_of(case):
        k = m - 1
        r = href.reference(*case, b, m)
        tag = "%s B=%d K=%d %s" % (case_id(case), b, k, tag_of(dtype))
        layers = layers_of(target, r["params"], steps, dtype)
        z, noise, unif = device_inputs(r, dtype)
        out, ld, trace, accept = annealed_kernel(target, layers, z, noise, unif, steps, r["betas"])
        again = annealed_kernel(target, layers, z, noise, unif, steps, r["betas"])
        plain = annealed_kernel(target, layers, z, noise, unif, steps, r["betas"], want_trace=False)
        assert all(torch.equal(x, y) for x, y in zip((out, ld, trace, accept), again)), tag + ": two calls differ"
        assert torch.equal(out, plain[0]) and torch.equal(ld, plain[1]), tag + ": the run depends on whether the trace is written"
        assert accept.dtype == torch.uint8 and tuple(accept.shape) == (k, b) and tuple(trace.shape) == (k, b, 2)
        assert torch.equal(trace[0], z) and int(accept.max()) <= 1
        keep = ~r["near"]
        assert sref.few_near(r["near"], k), "%s: %d rows in the band" % (tag, int(r["near"].sum()))
        differ = (accept.bool().cpu() != r[torch.float64][2]).any(0) & keep
        assert not differ.any(), "%s: %d rows outside the band decided differently" % (tag, int(differ.sum()))
        floors = (0.0, 0.0) if (b, m) == (1000, M) else (floor_of(case, 0), floor_of(case, 1))
        yard = href.reference(*case, 1000, m)["yardstick"]
        for j, (name, got) in enumerate((("z_out", out), ("log_det", ld))):
            judge(got.cpu()[keep], r[torch.float32][j][keep], r[torch.float64][j][keep], dtype, "%s %s" % (tag, name), floors[j], yard[j])
        for layer in range(k):                           # a rejected row is its entrance row bit for bit
            rejected = ~accept[layer].bool()
            after = trace[layer + 1] if layer + 1 < k else out
            assert torch.equal(after[rejected], trace[layer][rejected]), tag


# ---------------------------------------------------------------- 2. a run against its own layers, 5. logp_target
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", href.CASES, ids=case_id)
def test_run_is_its_layers_one_by_one(hip, case, dtype):
    """A K-layer launch against K launches of one layer, bit for bit: z_out, accept, the trace and the log_dets summed in
    layer order - the carried (log p, score) of the target is what a fresh evaluation gives.  And logp_target is the
    target kernel's log p at z_out."""
    family, n, steps, step = case
    target = target_of(family, n, dtype)
    for b, m in ((1000, M), (65, href.MS[1])):
        r = href.reference(*case, b, m)
        layers = layers_of(target, r["params"], steps, dtype)
        z, noise, unif = device_inputs(r, dtype)
        out, ld, trace, accept, lt = annealed_kernel(target, layers, z, noise, unif, steps, r["betas"], want_logp=True)
        x, total = z, None
        for k, layer in enumerate(layers):
            assert torch.equal(x, trace[k])
            x, one, _, acc = annealed_kernel(target, [layer], x, noise[k:k + 1], unif[k:k + 1], steps, r["betas"][k:k + 1])
            total = one if total is None else total + one
            assert torch.equal(acc[0], accept[k]), "layer %d decides differently on its own" % k
        assert torch.equal(x, out) and torch.equal(total, ld)
        table, scale = target._operands(z)
        assert torch.equal(lt, _lib.target_log_prob(out, target._family, table, scale)[0])
        assert torch.equal(lt, annealed_kernel(target, layers, z, noise, unif, steps, r["betas"], want_trace=False, want_logp=True)[2])


# ---------------------------------------------------------------- 3. beta = 1
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", href.CASES, ids=case_id)
def test_beta_one_is_the_plain_run(hip, case, dtype):
    """1 * lt + 0 * l0 is lt exactly: with beta = 1 in every layer the run and its gradients have the bits of
    vcnf_hmc_stack_* (the rows here are finite)."""
    family, n, steps, step = case
    target = target_of(family, n, dtype)
    r = href.reference(*case, 1000, M)
    layers = layers_of(target, r["params"], steps, dtype)
    z, noise, unif = device_inputs(r, dtype)
    ones = torch.ones(M - 1, dtype=dtype, device="cuda")
    table, scale = target._operands(z)
    loc, log_scale = prior_operands(dtype)
    g = torch.Generator().manual_seed(ref.seed_of("hais beta one", case))
    gz, gl = torch.randn(1000, 2, generator=g, dtype=torch.float64).to(dtype).cuda(), torch.randn(1000, generator=g, dtype=torch.float64).to(dtype).cuda()
    results = []
    for annealed in (True, False):
        x = z.clone().requires_grad_(True)
        for layer in layers:
            layer.zero_grad(set_to_none=True)
        step_, mass, sqm = fused_stochastic.operands(layers)
        if annealed:
            out, ld = nf.autograd.HmcAnnealedStackFn.apply(x, step_, mass, sqm, noise, unif, ones, loc, log_scale, steps, target._family, table, scale)
            accept = annealed_kernel(target, layers, z, noise, unif, steps, ones)[3]
        else:
            out, ld = nf.autograd.HmcStackFn.apply(x, step_, mass, sqm, noise, unif, steps, target._family, table, scale)
            accept = _lib.hmc_stack(z, noise, unif, step_.detach(), mass.detach(), sqm.detach(), steps, target._family, table, scale, want_trace=True)[3]
        torch.autograd.backward((out, ld), (gz, gl))
        results.append([out.detach(), ld.detach(), accept, x.grad] + [p.grad.clone() for layer in layers for p in (layer.log_step_size, layer.log_mass)])
    assert torch.isfinite(results[1][0]).all() and torch.isfinite(results[1][1]).all() and bool(results[1][2].any())
    for i, (a, c) in enumerate(zip(*results)):
        assert torch.equal(a, c), "output %d differs from the plain run's" % i


# ---------------------------------------------------------------- 4. beta = 0
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", sref.DEFAULTS, ids=case_id)
def test_beta_zero_is_the_prior(hip, tgt, dtype):
    """With beta = 0 the layer's density is the prior's; with unif = 0 every row whose probability is not 0 moves, and
    log_det is DiagGaussian.log_prob(z) - log_prob(z_out) of the package's own kernel to 4 eps."""
    family, n = tgt
    steps, step, b = 8, 0.1, 65
    target = target_of(family, n, dtype)
    r = href.reference(family, n, steps, step, b, 2)               # one layer
    layers = layers_of(target, r["params"], steps, dtype)
    z, noise, unif = device_inputs(r, dtype)
    out, ld, _, accept = annealed_kernel(target, layers, z, noise, torch.zeros_like(unif), steps, torch.zeros(1))
    assert int(accept.sum()) > b // 2 and bool((out != z).any())
    prior = prior_of(dtype)
    with torch.no_grad():
        lp, lp_out = prior.log_prob(z), prior.log_prob(out)
    eps = torch.finfo(dtype).eps
    bound = 4 * eps * torch.maximum(lp.abs(), lp_out.abs()) + 4 * eps
    err = (ld - (lp - lp_out)).abs()
    print("%s %s: log_det against the prior's kernel, max error %.3e (largest bound %.3e), %d of %d rows bitwise" % (
        case_id(tgt), tag_of(dtype), float(err.max()), float(bound.max()), int((ld == lp - lp_out).sum()), b))
    assert bool((err <= bound).all()), "%d rows outside 4 eps" % int((err > bound).sum())


# ---------------------------------------------------------------- 6. unusual rows
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", sref.DEFAULTS, ids=case_id)
def test_unusual_rows(hip, tgt, dtype):
    family, n = tgt
    steps, step, b = 8, 0.1, 65
    target = target_of(family, n, dtype)
    r = href.reference(family, n, steps, step, b, M)
    k, betas = M - 1, r["betas"]
    layers = layers_of(target, r["params"], steps, dtype)
    z, noise, unif = device_inputs(r, dtype)
    out, ld, trace, accept, lt = annealed_kernel(target, layers, z, noise, unif, steps, betas, want_logp=True)
    # a NaN row: NaN log_det, the row unchanged, the others as they were
    zn, nn_, un = ref.nan_row(z), torch.cat([noise, noise[:, :1]], 1), torch.cat([unif, unif[:, :1]], 1)
    outn, ldn, _, accn, ltn = annealed_kernel(target, layers, zn, nn_, un, steps, betas, want_logp=True)
    assert torch.equal(outn[:-1], out) and torch.equal(ldn[:-1], ld) and torch.equal(accn[:, :-1], accept) and torch.equal(ltn[:-1], lt)
    assert bool(torch.isnan(ldn[-1])) and bool(torch.isnan(outn[-1, 0])) and float(outn[-1, 1]) == 1.0 and not accn[:, -1].any()
    assert bool(torch.isnan(ltn[-1]))
    # steps = 0: z and zeros, whatever the draws
    same, zeros, _, acc = annealed_kernel(target, layers_of(target, r["params"], 0, dtype), z, noise, unif, 0, betas)
    assert torch.equal(same, z) and not zeros.any() and bool(acc.bool().all())
    # element accesses: z one element past its allocation's alignment gives the bits of the aligned call
    buf = torch.empty(2 * b + 1, dtype=dtype, device="cuda")
    buf[1:] = z.reshape(-1)
    shifted = buf[1:].view(b, 2)
    assert shifted.data_ptr() % (2 * z.element_size()) == z.element_size()
    outs, lds, traces, accs, lts = annealed_kernel(target, layers, shifted, noise, unif, steps, betas, want_logp=True)
    assert torch.equal(outs, out) and torch.equal(lds, ld) and torch.equal(accs, accept) and torch.equal(traces, trace) and torch.equal(lts, lt)
    # B = 0
    e = annealed_kernel(target, layers, z[:0], noise[:, :0], unif[:, :0], steps, betas, want_logp=True)
    assert [tuple(t.shape) for t in e] == [(0, 2), (0,), (k, 0, 2), (k, 0), (0,)]


def test_bad_arguments_raise(hip):
    target = target_of("circular", 8, torch.float32)
    f = lambda *shape, dtype=torch.float32: torch.ones(*shape, dtype=dtype, device="cuda")
    z = f(4, 2)
    table, scale = target._operands(z)
    good = dict(z=z, noise=f(2, 4, 2), unif=f(2, 4), step=f(2, 2), mass=f(2, 2), sqrt_mass=f(2, 2), beta=f(2), prior_loc=f(2),
                prior_log_scale=f(2))
    call = lambda steps=2, table=table, **kw: _lib.hmc_annealed_stack(*{**good, **kw}.values(), steps, target._family, table, scale)
    assert tuple(call()[0].shape) == (4, 2)
    for bad in (dict(z=f(4, 3)), dict(z=f(4)), dict(z=f(4, 2, dtype=torch.float16)), dict(z=torch.ones(4, 2)), dict(noise=f(2, 4, 3)),
                dict(noise=f(1, 4, 2)), dict(unif=f(2, 5)), dict(unif=f(2, 4, dtype=torch.float64)), dict(step=f(2)), dict(mass=f(3, 2)),
                dict(sqrt_mass=torch.ones(2, 2)), dict(beta=f(3)), dict(beta=f(2, 1)), dict(beta=f(2, dtype=torch.float64)),
                dict(beta=torch.ones(2)), dict(beta=None), dict(prior_loc=f(1, 2)), dict(prior_loc=f(3)), dict(prior_loc=None),
                dict(prior_log_scale=f(2, dtype=torch.float64)), dict(prior_log_scale=0.1), dict(steps=-1), dict(table=None),
                dict(table=table.double()), dict(steps=1 << 16)):
        with pytest.raises(nf.VcnfError):
            call(**bad)
    bwd = dict(trace=f(2, 4, 2), accept=torch.ones(2, 4, dtype=torch.uint8, device="cuda"), noise=f(2, 4, 2), step=f(2, 2), mass=f(2, 2),
               sqrt_mass=f(2, 2), beta=f(2), prior_loc=f(2), prior_log_scale=f(2))
    back = lambda steps=2, **kw: _lib.hmc_annealed_stack_bwd(*{**bwd, **kw}.values(), steps, target._family, table, scale, f(4, 2), f(4))
    assert [tuple(t.shape) for t in back()] == [(4, 2), (2, 2), (2, 2), (2, 2)]
    for bad in (dict(accept=f(2, 4)), dict(beta=f(1)), dict(beta=None), dict(prior_loc=f(2, dtype=torch.float64)), dict(prior_log_scale=f(3)),
                dict(noise=f(2, 5, 2)), dict(steps=1 << 16)):
        with pytest.raises(nf.VcnfError):
            back(**bad)


# ---------------------------------------------------------------- 7. gradients
def restatement_gradients(case, r, accept, gz, gl, dtype, numel=2, score=href.autograd_score):
    """(g_z, [g_log_step_size, g_log_mass per layer ...]) by autograd of the restatement in ``dtype`` on the CPU."""
    family, n, steps, step = case
    z = r["z"].to(dtype).clone().requires_grad_(True)
    params = [(ls[:numel].to(dtype).clone().requires_grad_(True), lm[:numel].to(dtype).clone().requires_grad_(True))
              for ls, lm in r["params"]]
    out, ld, _, _ = href.chain(family, n, z, r["noise"].to(dtype), r["unif"].to(dtype), params, steps, list(r["betas"]), score=score, accept=accept)
    leaves = [z] + [t for pair in params for t in pair]
    return torch.autograd.grad((out * gz.to(dtype)).sum() + (ld * gl.to(dtype)).sum(), leaves)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", href.CASES, ids=case_id)
def test_gradients(hip, case, dtype):
    """g_z, g_log_step_size and g_log_mass of the M = 4 chain at B = 1000 and of one layer at B = 65, with parameters of
    two elements and of one."""
    family, n, steps, step = case
    target = target_of(family, n, dtype)
    loc, log_scale = prior_operands(dtype)
    for b, m, numel in ((1000, M, 2), (65, 2, 2), (65, 2, 1)):
        k = m - 1
        r = href.reference(*case, b, m)
        tag = "%s B=%d K=%d numel=%d %s" % (case_id(case), b, k, numel, tag_of(dtype))
        g = torch.Generator().manual_seed(ref.seed_of("hais cotangent", case, b))
        gz, gl = torch.randn(b, 2, generator=g, dtype=torch.float64), torch.randn(b, generator=g, dtype=torch.float64)
        layers = layers_of(target, [(ls[:numel], lm[:numel]) for ls, lm in r["params"]], steps, dtype)
        z, noise, unif = device_inputs(r, dtype)
        betas = r["betas"].to(dtype).cuda()
        table, scale = target._operands(z)
        runs = []
        for _ in range(2):
            x = z.clone().requires_grad_(True)
            for layer in layers:
                layer.zero_grad(set_to_none=True)
            step_, mass, sqm = fused_stochastic.operands(layers)
            out, ld = nf.autograd.HmcAnnealedStackFn.apply(x, step_, mass, sqm, noise, unif, betas, loc, log_scale, steps, target._family, table, scale)
            assert type(out.grad_fn).__name__.startswith("HmcAnnealedStackFn")                  # ONE node
            ((out * gz.to(dtype).cuda()).sum() + (ld * gl.to(dtype).cuda()).sum()).backward()
            runs.append([x.grad.clone()] + [p.grad.clone() for layer in layers for p in (layer.log_step_size, layer.log_mass)])
        assert all(torch.equal(a, c) for a, c in zip(*runs)), tag + ": two backward calls differ"
        accept = annealed_kernel(target, layers, z, noise, unif, steps, r["betas"])[3].bool().cpu()
        want32 = restatement_gradients(case, r, accept, gz, gl, torch.float32, numel)
        want64 = restatement_gradients(case, r, accept, gz, gl, torch.float64, numel)
        closed = restatement_gradients(case, r, accept, gz, gl, torch.float64, numel, score=href.closed_form_score)
        names = ["g_z"] + ["g_%s[%d]" % (p, i) for i in range(k) for p in ("log_step_size", "log_mass")]
        for name, got, w32, w64, c64 in zip(names, runs[0], want32, want64, closed):
            assert tuple(got.shape) == tuple(w64.shape) and bool((got != 0).any()), "%s %s" % (tag, name)
            judge(got, w32, w64, dtype, "%s %s" % (tag, name), yardstick=float((c64 - w64).abs().max()))


# ---------------------------------------------------------------- 8. the modules
def sampler_of(target, prior, dtype, m, steps, step, fuse=True, device="cpu"):
    betas = href.betas_of(m, dtype).to(device)
    step_size = torch.tensor([step, 1.2 * step], dtype=dtype, device="cuda")
    log_mass = torch.tensor([0.1, -0.2], dtype=dtype, device="cuda")
    return nf.sampling.HAIS(betas, prior, target, steps, step_size, log_mass, fuse=fuse), step_size, log_mass


def count_launches(monkeypatch):
    calls = []
    launch = _lib.hmc_annealed_stack
    monkeypatch.setattr(_lib, "hmc_annealed_stack", lambda *a, **kw: calls.append(a[3].shape[0]) or launch(*a, **kw))
    return calls


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", [("two_moons", 0, 5, 0.1), ("circular", 8, 5, 0.1), ("ring", 2, 4, 0.3)], ids=case_id)
def test_hais_sample(hip, case, dtype, monkeypatch):
    family, n, steps, step = case
    m, num = 6, 1000
    k = m - 1
    target, prior = target_of(family, n, dtype), prior_of(dtype)
    calls = count_launches(monkeypatch)
    results = {}
    for device in ("cpu", "cuda"):                       # the alphas as host tensors and as device tensors
        for fuse in (True, False):
            sampler, step_size, log_mass = sampler_of(target, prior, dtype, m, steps, step, fuse, device)
            assert all(fused_stochastic.covers(layer, torch.zeros(1, 2, dtype=dtype, device="cuda")) for layer in sampler.layers)
            del calls[:]
            torch.manual_seed(23)
            with torch.no_grad():
                results[device, fuse] = sampler.sample(num)
            assert calls == ([k] if fuse else [1] * k), "fuse=%s: annealed launches %s" % (fuse, calls)
    samples, log_w = results["cpu", True]
    assert samples.dtype == dtype and tuple(samples.shape) == (num, 2) and tuple(log_w.shape) == (num,)
    for key, (s, w) in results.items():
        assert torch.equal(s, samples) and torch.equal(w, log_w), "%s differs: %d rows, %d weights" % (
            key, int((s != samples).any(1).sum()), int((w != log_w).sum()))
    # the module's draws, regenerated in the reference's order, given to the restatement's loop on the CPU
    torch.manual_seed(23)
    eps = torch.randn(num, 2, dtype=dtype, device="cuda")
    noise, unif = torch.empty(k, num, 2, dtype=dtype, device="cuda"), torch.empty(k, num, dtype=dtype, device="cuda")
    for j in range(k):
        noise[j] = torch.randn(num, 2, dtype=dtype, device="cuda")
        unif[j] = torch.rand(num, dtype=dtype, device="cuda")
    betas = href.layer_betas(m)

    def restatement(d, score=href.autograd_score):
        loc, log_scale = href.prior_parameters(d)
        x = loc + torch.exp(log_scale) * eps.cpu().to(d)
        params = [(torch.log(step_size).cpu().to(d), log_mass.cpu().to(d))] * k
        return href.hais_weights(family, n, x, href.prior_log_prob(x, loc, log_scale), noise.cpu().to(d), unif.cpu().to(d), params, steps, betas, score)

    r32, r64, closed = restatement(torch.float32), restatement(torch.float64), restatement(torch.float64, href.closed_form_score)
    near = ((torch.clamp(r64[3], max=2.0) - unif.cpu().double()).abs() < sref.HMC_BAND).any(0)
    keep = ~near
    assert sref.few_near(near, k), "%d rows in the band" % int(near.sum())
    tag = "%s HAIS %s" % (case_id(case), tag_of(dtype))
    print("%s: accepted per layer %s %%, %d rows in the band" % (tag, [round(100 * float(a), 1) for a in r64[2].double().mean(1)], int(near.sum())))
    yard = [float((closed[j] - r64[j])[keep].abs().max()) for j in (0, 1)]
    judge(samples.cpu()[keep], r32[0][keep], r64[0][keep], dtype, tag + " samples", yardstick=yard[0])
    judge(log_w.cpu()[keep], r32[1][keep], r64[1][keep], dtype, tag + " log_weights", yardstick=yard[1])
    # log Z from the rows outside the band: |logsumexp(a) - logsumexp(b)| <= max |a - b|, the largest of the per-row
    # tolerances that judge has just applied (and so under their sum)
    log_z = lambda w: float(torch.logsumexp(w.double(), 0)) - math.log(len(w))
    got_z, want_z, want32_z = log_z(log_w.cpu()[keep]), log_z(r64[1][keep]), log_z(r32[1][keep])
    if dtype == torch.float64:
        bound = 16.0 * yard[1] + 1e-12 * float(r64[1][keep].abs().max())
    else:
        bound = float((2e-5 + 2e-5 * r32[1][keep].abs().double()).max()) + 9.0 * float((r32[1][keep].double() - r64[1][keep]).abs().max())
    print("%s: log Z %.6f, the restatement's %.6f (fp32 %.6f), bound %.3e" % (tag, got_z, want_z, want32_z, bound))
    assert abs(got_z - want_z) <= bound
    ess = float(torch.exp(2 * torch.logsumexp(log_w.double(), 0) - torch.logsumexp(2 * log_w.double(), 0)))
    assert 1.0 <= ess <= num


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_trainable_prior_takes_the_torch_path_under_autograd(hip, dtype, monkeypatch):
    """The kernel has no gradient for the prior: while autograd records, a prior whose parameters require grad sends the
    layers to their torch composition, and the weights carry a gradient to the prior; without autograd it is one launch."""
    target, prior = target_of("two_moons", 0, dtype), prior_of(dtype, trainable=True)
    sampler, _, _ = sampler_of(target, prior, dtype, 4, 2, 0.1)
    calls = count_launches(monkeypatch)
    z = torch.zeros(3, 2, dtype=dtype, device="cuda")
    assert not any(fused_stochastic.covers(layer, z) for layer in sampler.layers)
    with torch.no_grad():
        assert all(fused_stochastic.covers(layer, z) for layer in sampler.layers)
        torch.manual_seed(5)
        sampler.sample(64)
    assert calls == [3]
    del calls[:]
    torch.manual_seed(5)
    samples, log_w = sampler.sample(64)
    assert calls == [] and log_w.requires_grad
    log_w.sum().backward()
    assert torch.isfinite(prior.loc.grad).all() and bool((prior.loc.grad != 0).any()) and bool((prior.log_scale.grad != 0).any())
    assert all(torch.isfinite(layer.log_step_size.grad).all() for layer in sampler.layers)
    # a frozen prior under autograd: one launch, one node, and the last term from target.log_prob
    frozen, _, _ = sampler_of(target, prior_of(dtype), dtype, 4, 2, 0.1)
    torch.manual_seed(5)
    samples, log_w = frozen.sample(64)
    assert calls == [3] and log_w.requires_grad
    log_w.sum().backward()
    assert all(torch.isfinite(p.grad).all() and bool((p.grad != 0).any()) for layer in frozen.layers for p in layer.parameters())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("tgt", sref.DEFAULTS, ids=case_id)
def test_model_with_annealed_layers(hip, tgt, dtype, monkeypatch):
    """A NormalizingFlow with annealed layers among its flows: the planner forms the annealed run - and keeps it apart
    from a plain HMC layer of the same target - in sample, log_prob and reverse_kld, and a step trains the step sizes."""
    family, n = tgt
    target, prior = target_of(family, n, dtype), prior_of(dtype)
    torch.manual_seed(43)
    params = sref.hmc_parameters(0.05, 4)
    bridges = [nf.distributions.LinearInterpolation(target, prior, beta) for beta in (0.25, 0.5, 0.75)]
    flows = [nf.flows.Planar(2, act="leaky_relu") for _ in range(2)] + \
            [nf.flows.HamiltonianMonteCarlo(t, 5, ls.float(), lm.float()) for t, (ls, lm) in zip(bridges + [target], params)]
    model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), flows, p=target)
    model = (model.double() if dtype == torch.float64 else model).cuda()
    assert len([k for k, _ in model.named_parameters() if "log_" in k and k.startswith("flows.")]) == 8
    calls = count_launches(monkeypatch)
    plain = []
    launch = _lib.hmc_stack
    monkeypatch.setattr(_lib, "hmc_stack", lambda *a, **kw: plain.append(a[3].shape[0]) or launch(*a, **kw))
    results = {}
    for fuse in (True, False):
        model.fuse_stochastic_stacks = fuse
        for name, call in (("sample", lambda: model.sample(1024)),
                           ("log_prob", lambda: (None, model.log_prob(href.inputs(family, n, 1000)[1].to(dtype).cuda())))):
            del calls[:], plain[:]
            torch.manual_seed(7)
            with torch.no_grad():
                results[name, fuse] = call()
            assert calls == ([3] if fuse else [1, 1, 1]) and plain == [1], "%s fuse=%s: launches %s, %s" % (name, fuse, calls, plain)
    model.fuse_stochastic_stacks = True
    z, log_q = results["sample", True]
    z1, log_q1 = results["sample", False]
    assert z.dtype == dtype and tuple(z.shape) == (1024, 2) and torch.isfinite(z).all() and torch.equal(z, z1)
    eps = torch.finfo(dtype).eps
    for a, c in ((log_q, log_q1), (results["log_prob", True][1], results["log_prob", False][1])):
        ok = torch.isfinite(c)
        assert torch.equal(torch.isfinite(a), ok) and bool(((a - c)[ok].abs() <= 64 * eps * (1 + c[ok].abs())).all())
    hmc = [(k, p) for k, p in model.named_parameters() if "log_" in k and k.startswith("flows.") and int(k.split(".")[1]) < 5]
    assert len(hmc) == 6
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        del calls[:], plain[:]
        torch.manual_seed(9)
        loss = model.reverse_kld(512)
        loss.backward()
        assert calls == [3] and plain == [1] and loss.dtype == dtype and bool(torch.isfinite(loss))
        runs.append([p.grad.clone() for p in model.parameters()])
    assert all(torch.isfinite(g).all() for g in runs[0]) and all(torch.equal(a, c) for a, c in zip(*runs))
    for k, p in hmc:                                     # the bridges are not the objective's target: nothing telescopes
        assert bool((p.grad != 0).all()), "%s: %s" % (k, p.grad.tolist())
    before = [p.detach().clone() for _, p in hmc]
    torch.optim.SGD(model.parameters(), lr=1e-4).step()
    assert all(not torch.equal(a, p.detach()) for a, (_, p) in zip(before, hmc))


# ---------------------------------------------------------------- 9. past the grid caps
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_past_the_grid_caps(hip, dtype):
    """One batch of two trips of the whole forward grid and a ragged third, K = 2, steps = 1, forward and VJP: the rows
    of the first trip, across the boundary between trip 1 and trip 2, and of the last full trip with the tail, run again
    as batches of their own, give the same bits (the method of test_gpu_grid_caps.py)."""
    block, cap = gc.constant("stoch.block"), gc.constant("stoch.cap")
    assert (block, cap, gc.constant("stoch.bwd_cap")) == (256, 2048, 1024)
    b, k, steps = (2 * cap + 5) * block + 37, 2, 1       # the VJP's 1024 workgroups take four trips and a ragged fifth
    trip = cap * block
    windows = ((0, 257), (trip - 128, trip + 129), (b - trip - (b - 2 * trip), b))
    assert b * 2 * k < 12e6
    family, n = "ring", 2
    target = target_of(family, n, dtype)
    g = torch.Generator().manual_seed(ref.seed_of("hais grid caps"))
    loc, log_scale = prior_operands(dtype)
    z = (torch.randn(b, 2, generator=g, dtype=torch.float64).to(dtype).cuda() * torch.exp(log_scale) + loc)
    noise = torch.randn(k, b, 2, generator=g, dtype=torch.float64).to(dtype).cuda()
    unif = torch.rand(k, b, generator=g, dtype=torch.float64).to(dtype).cuda()
    gz, gl = torch.randn(b, 2, generator=g, dtype=torch.float64).to(dtype).cuda(), torch.randn(b, generator=g, dtype=torch.float64).to(dtype).cuda()
    layers = layers_of(target, sref.hmc_parameters(0.3, k), steps, dtype)
    betas = torch.tensor([0.3, 0.7], dtype=dtype, device="cuda")
    table, scale = target._operands(z)

    def run(lo, hi):
        x = z[lo:hi].clone().requires_grad_(True)
        for layer in layers:
            layer.zero_grad(set_to_none=True)
        step, mass, sqm = fused_stochastic.operands(layers)
        es, us = noise[:, lo:hi].contiguous(), unif[:, lo:hi].contiguous()
        out, ld = nf.autograd.HmcAnnealedStackFn.apply(x, step, mass, sqm, es, us, betas, loc, log_scale, steps, target._family, table, scale)
        torch.autograd.backward((out, ld), (gz[lo:hi], gl[lo:hi]))
        with torch.no_grad():
            fwd = _lib.hmc_annealed_stack(z[lo:hi], es, us, step, mass, sqm, betas, loc, log_scale, steps, target._family, table, scale,
                                          want_trace=True, want_logp=True)
        assert torch.equal(fwd[0], out.detach()) and torch.equal(fwd[1], ld.detach())
        return fwd, x.grad, [p.grad.clone() for layer in layers for p in (layer.log_step_size, layer.log_mass)]

    (out, ld, trace, accept, lt), g_z, g_params = run(0, b)
    assert torch.isfinite(out).all() and torch.isfinite(ld).all() and torch.isfinite(g_z).all()
    assert 0.2 < float(accept.double().mean()) < 0.999 and all(torch.isfinite(p).all() and bool((p != 0).all()) for p in g_params)
    again = run(0, b)
    assert torch.equal(again[1], g_z) and all(torch.equal(a, c) for a, c in zip(again[2], g_params)), "two backward calls differ"
    for lo, hi in windows:
        (o, l, t, a, p), gzs, _ = run(lo, hi)
        for name, full, sub in (("z_out", out[lo:hi], o), ("log_det", ld[lo:hi], l), ("trace", trace[:, lo:hi], t),
                                ("accept", accept[:, lo:hi], a), ("logp_target", lt[lo:hi], p), ("g_z", g_z[lo:hi], gzs)):
            assert torch.equal(full, sub), "%s of the rows %d..%d differs when they are a batch of their own (%d elements)" % (
                name, lo, hi, int((full != sub).sum()))
