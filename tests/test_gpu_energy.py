"""The energy densities on the GPU (csrc/target_math.hpp through target_density.hip and stochastic.hip, the modules of
vcnf_amd.distributions.prior, the stochastic layers, HAIS and NormalizingFlow) against the plain-torch restatement
energy_ref.py run on the CPU, with the conventions of test_gpu_target.py, test_gpu_stochastic.py and test_gpu_hais.py:

* batches of a single row, a partial wave, an exact wave, a wave + 1 and a partial last workgroup;
* fp32 results are judged by helpers.parity against the restatement's fp32 run with its own fp32-vs-fp64 noise as the
  yardstick, the noise of the B = 1000 case of the same configuration as noise_floor for the smaller batches;
* fp64 densities by assert_close at 1e-10, their gradients at 1e-9 of the case's largest entry; fp64 results of the
  stochastic layers within 16 times the difference of the fp64 restatement run with autograd scores and with the
  closed-form scores of include/vcnf_hip.h, plus 1e-12 of the largest entry;
* decisions must be the fp64 restatement's on every row outside the near-tie band; rows inside it are left out of the value
  comparisons, and test_energy_ref.py pins on the CPU how few there are.

Measured on an MI355X, the largest figure over all cases: the fp64 kernels are within 2.3e-13 (log p), 2.9e-14 (score),
9.8e-13 (HMC z_out), 5.9e-12 (log_det), 8.9e-12 (g_z) and 1.0e-10 (parameter gradients) of the fp64 restatement; the fp32
kernels' largest errors against it are 8.1e-5, 6.4e-5, 1.4e-3, 2.1e-2, 2.0e-2 and 0.22 where the fp32 restatement's own
are 8.1e-5, 6.4e-5, 1.3e-3, 1.3e-2, 2.0e-2 and 0.23; no decision outside the band differs."""
import functools

import pytest
import torch

import energy_ref as eref
import target_ref as ref
import vcnf_amd as nf
from helpers import assert_close, parity
from vcnf_amd import _lib, fused_stochastic
from vcnf_amd.flows import Planar

pytestmark = pytest.mark.gpu

DTYPES = list(eref.DTYPES)
IDS = ["fp32", "fp64"]
F64 = dict(rtol=1e-10, atol=1e-10)
case_id = eref.case_id
tag_of = lambda dtype: IDS[DTYPES.index(dtype)]


# ---------------------------------------------------------------- the density
@functools.lru_cache(maxsize=None)
def reference(case, b):
    """{dtype: (log p, score, d (g . log p) / d z, log p with the NaN row appended)} of the restatement on the CPU, and
    the inputs.  Shared between tests: do not modify."""
    z, g = eref.inputs(case, b)
    out = {"z": z, "g": g}
    for dtype in DTYPES:
        lp, score, grad = eref.gradients(case, z, g, dtype)
        with torch.no_grad():
            lp_nan = eref.log_prob(case, ref.nan_row(z.to(dtype)))
        assert torch.isfinite(lp).all() and torch.isfinite(score).all() and torch.isfinite(grad).all()
        # torch's vectorised sigmoid on the CPU rounds a row in the vector body and in the scalar tail differently, and the
        # appended row moves rows between the two: the restatement agrees with itself to an ulp, the kernel bit for bit
        assert torch.isnan(lp_nan[-1]) and bool(((lp_nan[:-1] - lp).abs() <= 2 * torch.finfo(dtype).eps * lp.abs()).all())
        out[dtype] = (lp, score, grad, lp_nan)
    return out


def floors(case, b):
    if b == 1000:
        return (0.0, 0.0, 0.0, 0.0)
    big = reference(case, 1000)
    return tuple(float((big[torch.float32][j].double() - big[torch.float64][j])[:1000].abs().max()) for j in range(4))


def largest(case, j):
    return float(reference(case, 1000)[torch.float64][j].abs().max())


def judge_density(got, r, j, dtype, what, noise_floor=0.0, gradient=False, largest_entry=0.0):
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
@pytest.mark.parametrize("case", eref.CASES, ids=case_id)
def test_log_prob_score_and_gradient(hip, case, dtype):
    prior = eref.prior_of(case)
    for b in eref.BATCHES:
        r = reference(case, b)
        nf_lp, nf_score, nf_grad, nf_nan = floors(case, b)
        tag = "%s B=%d %s" % (case_id(case), b, tag_of(dtype))
        z = r["z"].to(dtype).cuda()
        with torch.no_grad():
            lp = prior.log_prob(z)
            score = prior.score(z)
            lp_nan = prior.log_prob(ref.nan_row(z))
            score_nan = prior.score(ref.nan_row(z))
        x = z.clone().requires_grad_(True)
        lp_graph = prior.log_prob(x)
        assert lp_graph.grad_fn is not None and type(lp_graph.grad_fn).__name__.startswith("TargetLogProbFn")   # ONE node
        grad, = torch.autograd.grad((r["g"].to(dtype).cuda() * lp_graph).sum(), x)
        for j, (name, t) in enumerate((("log_prob", lp), ("score", score), ("gradient", grad))):
            err, noise = ((v.detach().cpu().double() - r[torch.float64][j]).abs().max() for v in (t, r[torch.float32][j]))
            print("%s %s: max |got - fp64 restatement| %.3e (the fp32 restatement's %.3e)" % (tag, name, float(err), float(noise)))
        judge_density(lp, r, 0, dtype, tag + " log_prob", nf_lp)
        judge_density(score, r, 1, dtype, tag + " score", nf_score, gradient=True, largest_entry=largest(case, 1))
        judge_density(grad, r, 2, dtype, tag + " gradient", nf_grad, gradient=True, largest_entry=largest(case, 2))
        judge_density(lp_nan, r, 3, dtype, tag + " log_prob with a NaN row", nf_nan)
        assert torch.equal(lp_graph.detach(), lp), tag + ": log_prob differs under autograd"
        assert torch.equal(lp_nan[:-1], lp) and bool(torch.isnan(lp_nan[-1])) and bool(torch.isnan(score_nan[-1]).all())
        assert torch.equal(score_nan[:-1], score)
        assert r["z"][0].tolist() == [0.0, 0.0] and torch.isfinite(score[0]).all() and torch.isfinite(grad[0]).all()
        if case[0] in ("two_modes", "smiley"):           # r == 0 and sign(0) = 0: exactly the restatement's 0
            assert float(score[0, 0]) == 0.0 == float(r[torch.float64][1][0, 0])
    # Smiley's kink (1, -0.8): in fp64 z1 + 0.8 is exactly 0 there and the |.| term adds exactly nothing to the score
    if case[0] == "smiley" and dtype == torch.float64:
        z = reference(case, 1000)["z"][7:8].cuda()
        radius = float(torch.sqrt((z ** 2).sum()))
        assert abs(float(prior.score(z)[0, 1]) - (-(radius - 2) / 0.16 * (-0.8 / radius))) <= 1e-14


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", eref.CASES, ids=case_id)
def test_misaligned_rows_and_scoreless_path(hip, case, dtype):
    """z one element past its allocation takes the element loads; the launch without a score is another kernel instance.
    Both give the bits of the aligned launch with a score."""
    prior = eref.prior_of(case)
    for b in (65, 1000):
        z = reference(case, b)["z"].to(dtype).cuda()
        buf = torch.empty(2 * b + 1, dtype=dtype, device="cuda")
        buf[1:] = z.reshape(-1)
        shifted = buf[1:2 * b + 1].view(b, 2)
        width = 2 * z.element_size()
        assert shifted.is_contiguous() and z.data_ptr() % width == 0 and shifted.data_ptr() % width == z.element_size()
        table, scale = prior._operands(z)
        with torch.no_grad():
            lp, score = _lib.target_log_prob(z, prior._family, table, scale, want_score=True)
            lp_plain, none = _lib.target_log_prob(z, prior._family, table, scale)
            lp_shift, score_shift = _lib.target_log_prob(shifted, prior._family, table, scale, want_score=True)
            lp_shift_plain, _ = _lib.target_log_prob(shifted, prior._family, table, scale)
            assert none is None and torch.isfinite(lp).all()
            assert torch.equal(lp, lp_plain), "log_prob depends on whether the score is written"
            assert torch.equal(lp, lp_shift) and torch.equal(score, score_shift) and torch.equal(lp, lp_shift_plain)
            assert torch.equal(prior.log_prob(shifted), lp) and torch.equal(prior.score(shifted), score)
            wide = torch.zeros(b, 4, dtype=dtype, device="cuda")     # a non-contiguous view is made contiguous
            wide[:, 1:3] = z
            assert torch.equal(prior.log_prob(wide[:, 1:3]), lp)


def test_other_inputs_take_the_torch_composition(hip):
    """Half precision, other shapes and host tensors evaluate the torch composition on their own device; a reassigned
    attribute reaches the kernel."""
    for case in eref.FAMILIES:
        prior = eref.prior_of(case)
        z = reference(case, 65)["z"].float().cuda()
        want = prior.log_prob(z)
        half = prior.log_prob(z.half())
        assert half.dtype == torch.float16 and half.is_cuda and tuple(half.shape) == (65,)
        assert_close(prior.log_prob(z.cpu()), want, rtol=1e-4, atol=1e-4, what="host tensor")
        if case[0] in ("sinusoidal", "gap", "split"):
            assert_close(prior.log_prob(z[:60].reshape(3, 20, 2)), want[:60].reshape(3, 20), rtol=1e-4, atol=1e-4, what="rank 3")
        assert tuple(prior.log_prob(torch.zeros(0, 2, device="cuda")).shape) == (0,)
        prior.scale = 2 * prior.scale
        other = eref.prior_of((case[0], tuple(2 * p if i == (1 if case[0] == "two_modes" else 0) else p for i, p in enumerate(case[1]))))
        assert torch.equal(prior.log_prob(z), other.log_prob(z)) and not torch.equal(prior.log_prob(z), want)


# ---------------------------------------------------------------- HMC
def layers_of(target, params, steps, dtype):
    return [nf.flows.HamiltonianMonteCarlo(target, steps, ls.to(dtype), lm.to(dtype)).cuda() for ls, lm in params]


def prior_operands(dtype):
    return torch.tensor(eref.LOC, dtype=dtype).cuda(), torch.tensor(eref.LOG_SCALE, dtype=dtype).cuda()


def hmc_kernel(target, layers, z, noise, unif, steps, betas=None, want_trace=True, want_logp=False):
    """The plain run, or with ``betas`` the annealed one."""
    table, scale = target._operands(z)
    with torch.no_grad():
        step, mass, sqm = fused_stochastic.operands(layers)
        if betas is None:
            return _lib.hmc_stack(z, noise, unif, step, mass, sqm, steps, target._family, table, scale, want_trace=want_trace)
        loc, log_scale = prior_operands(z.dtype)
        return _lib.hmc_annealed_stack(z, noise, unif, step, mass, sqm, torch.tensor(betas, dtype=z.dtype).cuda(), loc, log_scale, steps,
                                       target._family, table, scale, want_trace=want_trace, want_logp=want_logp)


def judge(got, r32, r64, dtype, what, noise_floor=0.0, yardstick=0.0):
    """fp32: helpers.parity; fp64: |got - r64| <= 16 yardstick + 1e-12 max|r64|."""
    got = got.detach().cpu()
    assert got.dtype == dtype and got.shape == r64.shape, what
    err = float((got.double() - r64).abs().max()) if got.numel() else 0.0
    print("%s: max |got - fp64 restatement| %.3e (the fp32 restatement's %.3e)" % (
        what, err, float((r32.double() - r64).abs().max()) if got.numel() else 0.0))
    if dtype == torch.float32:
        parity(got, r32, r64, what=what, noise_floor=noise_floor)
    else:
        bound = 16.0 * yardstick + 1e-12 * float(r64.abs().max())
        assert torch.isfinite(got).all() and err <= bound, "%s: %.3e > %.3e" % (what, err, bound)


def hmc_floor(case, steps, step, k, j, annealed):
    """Noise of quantity j (0 z_out, 1 log_det) on the kept rows of the B = 1000 case of the same kind."""
    big = eref.hmc_reference(case, steps, step, 1000, 1 if not annealed else k, annealed)
    return float((big[torch.float32][j].double() - big[torch.float64][j])[~big["near"]].abs().max())


def check_run(case, dtype, steps, step, b, k, annealed):
    target = eref.prior_of(case)
    r = eref.hmc_reference(case, steps, step, b, k, annealed)
    k = len(r["params"])
    tag = "%s steps %d step %g B=%d K=%d%s %s" % (case_id(case), steps, step, b, k, " annealed" if annealed else "", tag_of(dtype))
    layers = layers_of(target, r["params"], steps, dtype)
    z, noise, unif = (r[name].to(dtype).cuda() for name in ("z", "noise", "unif"))
    out, ld, trace, accept = hmc_kernel(target, layers, z, noise, unif, steps, r["betas"])
    again = hmc_kernel(target, layers, z, noise, unif, steps, r["betas"])
    plain = hmc_kernel(target, layers, z, noise, unif, steps, r["betas"], want_trace=False)
    assert all(torch.equal(x, y) for x, y in zip((out, ld, trace, accept), again)), tag + ": two calls differ"
    assert torch.equal(out, plain[0]) and torch.equal(ld, plain[1]), tag + ": the run depends on whether the trace is written"
    assert accept.dtype == torch.uint8 and tuple(accept.shape) == (k, b) and tuple(trace.shape) == (k, b, 2)
    assert torch.equal(trace[0], z) and int(accept.max()) <= 1
    keep = ~r["near"]
    assert eref.few_near(r["near"], k), "%s: %d rows in the band" % (tag, int(r["near"].sum()))
    differ = (accept.bool().cpu() != r[torch.float64][2]).any(0) & keep
    assert not differ.any(), "%s: %d rows outside the band decided differently" % (tag, int(differ.sum()))
    floors_ = (0.0, 0.0) if b == 1000 else tuple(hmc_floor(case, steps, step, k, j, annealed) for j in (0, 1))
    yard = eref.hmc_reference(case, steps, step, 1000, k, annealed)["yardstick"]
    for j, (name, got) in enumerate((("z_out", out), ("log_det", ld))):
        judge(got.cpu()[keep], r[torch.float32][j][keep], r[torch.float64][j][keep], dtype, "%s %s" % (tag, name), floors_[j], yard[j])
    for layer in range(k):                               # a rejected row is its entrance row bit for bit
        rejected = ~accept[layer].bool()
        after = trace[layer + 1] if layer + 1 < k else out
        assert torch.equal(after[rejected], trace[layer][rejected]), tag
    if k == 1 and not annealed:
        assert not ld[~accept[0].bool()].any(), tag
    return r, layers, (z, noise, unif), (out, ld, trace, accept)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("steps", eref.HMC_STEPS, ids=case_id)
@pytest.mark.parametrize("case", eref.CASES, ids=case_id)
def test_hmc_forward(hip, case, steps, dtype):
    for b, k in eref.hmc_runs():
        check_run(case, dtype, *steps, b, k, False)


def restatement_gradients(case, r, steps, accept, gz, gl, dtype, closed=False):
    """(g_z, g_log_step_size[0], g_log_mass[0], ...) of the restatement's closed-form backward in ``dtype`` on the CPU."""
    k = len(r["params"])
    dens = eref.densities(case, k, r["betas"], closed)
    params = [(ls.to(dtype), lm.to(dtype)) for ls, lm in r["params"]]
    g_z, grads = eref.hmc_backward(dens, r["z"].to(dtype), r["noise"].to(dtype), params, steps, accept, gz.to(dtype), gl.to(dtype))
    return [g_z] + [t for pair in grads for t in pair]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("annealed", [False, True], ids=["plain", "annealed"])
@pytest.mark.parametrize("steps", eref.HMC_STEPS, ids=case_id)
@pytest.mark.parametrize("case", eref.FAMILIES, ids=case_id)
def test_hmc_gradients(hip, case, steps, annealed, dtype):
    """g_z, g_log_step_size and g_log_mass of a run at B = 1000 and of one layer at B = 65 (the annealed chain at both)
    against the restatement's closed-form backward with the kernel's own decisions imposed, so that a band row cannot
    become a gradient mismatch."""
    target = eref.prior_of(case)
    steps, step = steps
    for b, k in (((1000, eref.M - 1), (65, eref.M - 1)) if annealed else ((1000, eref.RUN), (65, 1))):
        r = eref.hmc_reference(case, steps, step, b, k, annealed)
        tag = "%s steps %d B=%d K=%d%s %s" % (case_id(case), steps, b, k, " annealed" if annealed else "", tag_of(dtype))
        g = torch.Generator().manual_seed(ref.seed_of("energy cotangent", case, b))
        gz, gl = torch.randn(b, 2, generator=g, dtype=torch.float64), torch.randn(b, generator=g, dtype=torch.float64)
        layers = layers_of(target, r["params"], steps, dtype)
        z, noise, unif = (r[name].to(dtype).cuda() for name in ("z", "noise", "unif"))
        table, scale = target._operands(z)
        runs = []
        for _ in range(2):
            x = z.clone().requires_grad_(True)
            for layer in layers:
                layer.zero_grad(set_to_none=True)
            step_, mass, sqm = fused_stochastic.operands(layers)
            if annealed:
                out, ld = nf.autograd.HmcAnnealedStackFn.apply(x, step_, mass, sqm, noise, unif, torch.tensor(r["betas"], dtype=dtype).cuda(),
                                                               *prior_operands(dtype), steps, target._family, table, scale)
            else:
                out, ld = nf.autograd.HmcStackFn.apply(x, step_, mass, sqm, noise, unif, steps, target._family, table, scale)
            assert type(out.grad_fn).__name__.startswith("HmcAnnealedStackFn" if annealed else "HmcStackFn")      # ONE node
            ((out * gz.to(dtype).cuda()).sum() + (ld * gl.to(dtype).cuda()).sum()).backward()
            runs.append([x.grad.clone()] + [p.grad.clone() for layer in layers for p in (layer.log_step_size, layer.log_mass)])
        assert all(torch.equal(a, c) for a, c in zip(*runs)), tag + ": two backward calls differ"
        accept = hmc_kernel(target, layers, z, noise, unif, steps, r["betas"])[3].bool().cpu()
        want32 = restatement_gradients(case, r, steps, accept, gz, gl, torch.float32)
        want64 = restatement_gradients(case, r, steps, accept, gz, gl, torch.float64)
        closed = restatement_gradients(case, r, steps, accept, gz, gl, torch.float64, closed=True)
        names = ["g_z"] + ["g_%s[%d]" % (p, i) for i in range(k) for p in ("log_step_size", "log_mass")]
        for name, got, w32, w64, c64 in zip(names, runs[0], want32, want64, closed):
            assert tuple(got.shape) == tuple(w64.shape) and bool((got != 0).any()), "%s %s" % (tag, name)
            judge(got, w32, w64, dtype, "%s %s" % (tag, name), yardstick=float((c64 - w64).abs().max()))


# ---------------------------------------------------------------- MH
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", eref.CASES, ids=case_id)
def test_mh_walk(hip, case, dtype):
    target = eref.prior_of(case)
    for steps in eref.MH_STEPS:
        for scale in eref.MH_SCALES:
            big = eref.mh_reference(case, steps, scale, 1000)
            floor = float((big[torch.float32][0].double() - big[torch.float64][0])[~big["near"]].abs().max())
            for b in eref.MH_BATCHES:
                r = eref.mh_reference(case, steps, scale, b)
                tag = "%s steps %d scale %s B=%d %s" % (case_id(case), steps, scale, b, tag_of(dtype))
                z, eps, w = (r[name].to(dtype).cuda() for name in ("z", "eps", "w"))
                prop = torch.tensor(scale, dtype=dtype, device="cuda")
                table, tscale = target._operands(z)
                out, accept = _lib.mh_walk(z, eps, w, prop, target._family, table, tscale, want_accept=True)
                assert torch.equal(out, _lib.mh_walk(z, eps, w, prop, target._family, table, tscale)), tag
                keep = ~r["near"]
                assert eref.few_near(r["near"]), "%s: %d rows in the band" % (tag, int(r["near"].sum()))
                differ = (accept.bool().cpu() != r[torch.float64][1]).any(0) & keep
                assert not differ.any(), "%s: %d rows outside the band decided differently" % (tag, int(differ.sum()))
                judge(out.cpu()[keep], r[torch.float32][0][keep], r[torch.float64][0][keep], dtype, tag + " z_out",
                      0.0 if b == 1000 else floor)
                stay = ~accept.bool().any(0)
                assert torch.equal(out[stay], z[stay]), tag
    # the module: one launch, the draws in the reference's order, log_det exactly zero, the identity backwards
    prop = nf.distributions.DiagGaussianProposal((2,), [0.3, 0.24]).to(dtype).cuda()
    layer = nf.flows.MetropolisHastings(target, prop, 4)
    z = eref.rows(case, 1000).to(dtype).cuda()
    assert fused_stochastic.covers_walk(layer, z)
    assert not fused_stochastic.covers_walk(nf.flows.MetropolisHastings(eref.PlainEnergy(case), prop, 4), z)
    torch.manual_seed(29)
    x = z.clone().requires_grad_(True)
    out, ld = layer(x)
    assert ld.dtype == dtype and tuple(ld.shape) == (1000,) and not ld.any()
    torch.manual_seed(29)
    eps, w = torch.empty(4, 1000, 2, dtype=dtype, device="cuda"), torch.empty(4, 1000, dtype=dtype, device="cuda")
    for i in range(4):
        eps[i] = torch.randn((1000,) + prop.shape, dtype=dtype, device="cuda")
        w[i] = torch.rand(1000, dtype=dtype, device="cuda")
    table, tscale = target._operands(z)
    assert torch.equal(out.detach(), _lib.mh_walk(z, eps, w, prop.scale[0], target._family, table, tscale)), case_id(case)
    gz = torch.randn(1000, 2, dtype=dtype, device="cuda")
    grad, = torch.autograd.grad((out * gz).sum(), x)
    assert torch.equal(grad, gz)


# ---------------------------------------------------------------- annealed runs and HAIS
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("steps", eref.HMC_STEPS, ids=case_id)
@pytest.mark.parametrize("case", eref.FAMILIES, ids=case_id)
def test_annealed_run(hip, case, steps, dtype):
    """The chain of M - 1 annealed layers against the restatement; the target's log p at z_out from the same launch is the
    density kernel's; with beta = 1 in every layer the run has the plain run's bits."""
    for b, k in eref.hmc_runs(annealed=True):
        r, layers, (z, noise, unif), (out, ld, trace, accept) = check_run(case, dtype, *steps, b, k, True)
    target = eref.prior_of(case)
    lt = hmc_kernel(target, layers, z, noise, unif, steps[0], r["betas"], want_logp=True)[4]
    assert torch.equal(lt, target.log_prob(out))
    ones = hmc_kernel(target, layers, z, noise, unif, steps[0], (1.0,) * len(layers))
    plain = hmc_kernel(target, layers, z, noise, unif, steps[0])
    assert all(torch.equal(a, c) for a, c in zip(ones, plain)) and bool(plain[3].any())


def diag_gaussian(dtype):
    """The restatement's prior as the package's DiagGaussian on the device."""
    prior = nf.distributions.DiagGaussian(2, trainable=False)
    prior = (prior.double() if dtype == torch.float64 else prior).cuda()
    loc, log_scale = prior_operands(dtype)
    with torch.no_grad():
        prior.loc.copy_(loc.reshape(1, 2))
        prior.log_scale.copy_(log_scale.reshape(1, 2))
    return prior


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", eref.FAMILIES, ids=case_id)
def test_hais_sample(hip, case, dtype, monkeypatch):
    """HAIS.sample(1000) at 6 betas: one launch, the bits of its layers one by one under one seed, and the restatement's
    loop on the CPU with the same draws."""
    steps, step, m, num = 4, 0.3, 6, 1000
    k = m - 1
    target, prior = eref.prior_of(case), diag_gaussian(dtype)
    calls = []
    launch = _lib.hmc_annealed_stack
    monkeypatch.setattr(_lib, "hmc_annealed_stack", lambda *a, **kw: calls.append(a[3].shape[0]) or launch(*a, **kw))
    step_size = torch.tensor([step, 1.2 * step], dtype=dtype, device="cuda")
    log_mass = torch.tensor([0.1, -0.2], dtype=dtype, device="cuda")
    results = {}
    for fuse in (True, False):
        sampler = nf.sampling.HAIS(torch.linspace(1, 0, m + 1, dtype=dtype), prior, target, steps, step_size, log_mass, fuse=fuse)
        assert all(fused_stochastic.covers(layer, torch.zeros(1, 2, dtype=dtype, device="cuda")) for layer in sampler.layers)
        del calls[:]
        torch.manual_seed(23)
        with torch.no_grad():
            results[fuse] = sampler.sample(num)
        assert calls == ([k] if fuse else [1] * k), "fuse=%s: annealed launches %s" % (fuse, calls)
    samples, log_w = results[True]
    assert samples.dtype == dtype and tuple(samples.shape) == (num, 2) and tuple(log_w.shape) == (num,)
    assert torch.equal(samples, results[False][0]) and torch.equal(log_w, results[False][1])
    # the module's draws, regenerated in the reference's order, given to the restatement's loop on the CPU
    torch.manual_seed(23)
    eps = torch.randn(num, 2, dtype=dtype, device="cuda")
    noise, unif = torch.empty(k, num, 2, dtype=dtype, device="cuda"), torch.empty(k, num, dtype=dtype, device="cuda")
    for j in range(k):
        noise[j] = torch.randn(num, 2, dtype=dtype, device="cuda")
        unif[j] = torch.rand(num, dtype=dtype, device="cuda")
    betas = eref.layer_betas(m)

    def restatement(d, closed=False):
        loc, log_scale = torch.tensor(eref.LOC, dtype=d), torch.tensor(eref.LOG_SCALE, dtype=d)
        x = loc + torch.exp(log_scale) * eps.cpu().to(d)
        params = [(torch.log(step_size).cpu().to(d), log_mass.cpu().to(d))] * k
        out, ld, accept, prob = eref.hmc_run(eref.densities(case, k, betas, closed), x, noise.cpu().to(d), unif.cpu().to(d), params, steps)
        return out, -eref.prior_log_prob(x) + ld + eref.log_prob(case, out), accept, prob

    r32, r64, closed = restatement(torch.float32), restatement(torch.float64), restatement(torch.float64, True)
    near = ((torch.clamp(r64[3], max=2.0) - unif.cpu().double()).abs() < eref.HMC_BAND).any(0)
    keep = ~near
    assert eref.few_near(near, k), "%d rows in the band" % int(near.sum())
    tag = "%s HAIS %s" % (case_id(case), tag_of(dtype))
    print("%s: accepted per layer %s %%, %d rows in the band" % (tag, [round(100 * float(a), 1) for a in r64[2].double().mean(1)], int(near.sum())))
    yard = [float((closed[j] - r64[j])[keep].abs().max()) for j in (0, 1)]
    judge(samples.cpu()[keep], r32[0][keep], r64[0][keep], dtype, tag + " samples", yardstick=yard[0])
    judge(log_w.cpu()[keep], r32[1][keep], r64[1][keep], dtype, tag + " log_weights", yardstick=yard[1])


# ---------------------------------------------------------------- the model
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("case", eref.FAMILIES, ids=case_id)
def test_model_runs_fuse(hip, case, dtype, monkeypatch):
    """Consecutive HMC layers that share the object and the step count are one launch, plain and annealed, in a fp32 model
    and a .double() one; the torch path under the same seed walks the same chain up to decisions at near ties."""
    target = eref.prior_of(case)
    params = eref.hmc_parameters(0.05, eref.RUN)
    z = eref.rows(case, 1000).to(dtype).cuda()
    for annealed in (False, True):
        name = "hmc_annealed_stack" if annealed else "hmc_stack"
        calls = []
        launch = getattr(_lib, name)
        monkeypatch.setattr(_lib, name, lambda *a, _launch=launch, **kw: calls.append(a[3].shape[0]) or _launch(*a, **kw))
        prior = diag_gaussian(dtype)
        kernel_target = nf.distributions.LinearInterpolation(target, prior, 0.5) if annealed else target
        plain_energy = eref.PlainEnergy(case)
        plain_target = nf.distributions.LinearInterpolation(plain_energy, prior, 0.5) if annealed else plain_energy
        results = []
        for t in (kernel_target, plain_target):
            flows = [nf.flows.HamiltonianMonteCarlo(t, 5, ls.float(), lm.float()) for ls, lm in params]
            model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), flows)
            model = (model.double() if dtype == torch.float64 else model).cuda()
            torch.manual_seed(7)
            with torch.no_grad():
                results.append(model.log_prob(z))
        assert calls == [eref.RUN], "%s: launches %s" % (name, calls)
        monkeypatch.setattr(_lib, name, launch)
        # a row walks differently where one of its three decisions is near a tie: at most the cap's share per decision
        got, want = results
        ok = torch.isfinite(want)
        moved = (got - want).abs() > 1e-3 * (1 + want.abs())
        assert torch.equal(torch.isfinite(got), ok) and float(moved[ok].double().mean()) <= eref.RUN * eref.BAND_CAP, int(moved[ok].sum())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_reverse_kld_step(hip, dtype):
    """One reverse_kld step of a 4-layer Planar model with p = TwoModes / Sinusoidal: the loss and the parameter gradients
    are those of the same model whose p is the torch restatement.  The models share the seeds, so they draw the same
    samples.  fp32 is judged by helpers.parity with the restatement's own fp32 noise as the yardstick: the third model's p
    is the restatement evaluated in fp64 on the fp32 samples.  fp64: 1e-10 for the loss, 1e-9 of a gradient's largest
    entry."""
    for case in (("two_modes", (2.0, 0.2)), ("sinusoidal", (0.4, 4.0))):
        runs = []
        for p in (eref.prior_of(case), eref.PlainEnergy(case), eref.PlainEnergy(case, torch.float64), eref.prior_of(case)):
            torch.manual_seed(41)
            model = nf.NormalizingFlow(nf.distributions.DiagGaussian(2), [Planar(2) for _ in range(4)], p=p)
            model = (model.double() if dtype == torch.float64 else model).cuda()
            torch.manual_seed(7)
            loss = model.reverse_kld(256)
            loss.backward()
            runs.append([loss.detach().reshape(1)] + [q.grad.clone() for q in model.parameters()])
        got, want, wide, again = runs
        assert got[0].dtype == dtype and all(torch.equal(a, c) for a, c in zip(got, again))
        for i, (a, w, w64) in enumerate(zip(got, want, wide)):
            what = "%s %s %s" % (case_id(case), tag_of(dtype), "loss" if i == 0 else "gradient %d" % i)
            print("%s: max |got - restatement| %.3e of %.3e (the restatement's fp32 noise %.3e)" % (
                what, float((a - w).abs().max()), float(w.abs().max()), float((w - w64).abs().max())))
            assert torch.isfinite(a).all() and bool((a != 0).any()), what
            if dtype == torch.float32:
                parity(a, w.cpu(), w64.cpu(), what=what)
            elif i == 0:
                assert_close(a, w, what=what, **F64)
            else:
                assert float((a - w).abs().max()) <= 1e-9 * float(w.abs().max()), what
