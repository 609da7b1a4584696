"""Hamiltonian annealed importance sampling without a GPU: the vcnf_hmc_annealed_stack_* / _bwd_* prototypes are read
from include/vcnf_hip.h, exported, bound, and return the documented status codes before anything is launched; the _lib
wrappers refuse wrong shapes and dtypes; ``LinearInterpolation`` and ``HAIS`` carry the reference's structure and, on CPU
tensors with a plain-torch prior and a plain Target subclass, are the restatement (hais_ref.py) bit for bit under one
seed; the closed-form backward with score_k in place of the score is fp64 autograd of the restatement; and the near-tie
bands the GPU tests leave out are as thin as they assume.

Measured here: at most 0.96 % of a case's decisions lie in the band (2 % allowed); the rows left out at B = 1000 are at
most 3.6 % for the three-layer chains and 8.4 % for the eight-layer ones (few_near allows 6 % and 16 %)."""
import ctypes

import pytest
import torch

import hais_ref as href
import stochastic_ref as sref
import target_ref
import vcnf_amd as nf
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
case_id = lambda c: "-".join(str(x) for x in c) if isinstance(c, tuple) else str(c)

FWD_PTRS = ("z", "noise", "unif", "step", "mass", "sqrt_mass", "beta", "prior_loc", "prior_log_scale", "table", "z_out",
            "log_det", "logp_target", "trace", "accept")
BWD_PTRS = ("trace", "accept", "noise", "step", "mass", "sqrt_mass", "beta", "prior_loc", "prior_log_scale", "table", "g_out",
            "g_logdet", "g_in", "g_step", "g_mass", "g_sqrt_mass", "workspace")


def test_prototypes_come_from_the_header():
    handle = ctypes.CDLL(_lib.lib_path())
    for base, ptrs, ints in (("vcnf_hmc_annealed_stack", FWD_PTRS, 3), ("vcnf_hmc_annealed_stack_bwd", BWD_PTRS, 4)):
        for sfx, real in (("_f32", ctypes.c_float), ("_f64", ctypes.c_double)):
            name = base + sfx
            assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
            assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
            args = _lib.PROTOTYPES[name][0]
            assert len(args) == len(ptrs) + 1 + ints + 3             # pointers, batch, the int32s, family, scale, stream
            assert args[-2] is real                                  # the target's scale, before the stream
    # the plain entry points' argument lists with the three operands and the one output more
    assert len(_lib.PROTOTYPES["vcnf_hmc_annealed_stack_f32"][0]) == len(_lib.PROTOTYPES["vcnf_hmc_stack_f32"][0]) + 4
    assert len(_lib.PROTOTYPES["vcnf_hmc_annealed_stack_bwd_f32"][0]) == len(_lib.PROTOTYPES["vcnf_hmc_stack_bwd_f32"][0]) + 3
    assert callable(_lib.hmc_annealed_stack) and callable(_lib.hmc_annealed_stack_bwd)
    assert issubclass(nf.autograd.HmcAnnealedStackFn, torch.autograd.Function)


def _fwd(L, sfx, b=4, k=2, steps=3, n=3, family=1, **ptrs):
    return getattr(L, "vcnf_hmc_annealed_stack" + sfx)(*[ptrs.get(p, FAKE) for p in FWD_PTRS], b, k, steps, n, family, 0.5, None)


def _bwd(L, sfx, b=4, k=2, steps=3, groups=1, n=3, family=1, **ptrs):
    return getattr(L, "vcnf_hmc_annealed_stack_bwd" + sfx)(*[ptrs.get(p, FAKE) for p in BWD_PTRS], b, k, steps, groups, n, family,
                                                           0.5, None)


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    """check_run's and hmc_stack's checks in their order; beta and the prior's parameters are required and aligned."""
    L = nf.lib()
    for call, ptrs in ((_fwd, FWD_PTRS), (_bwd, BWD_PTRS)):
        optional = {"logp_target", "trace", "accept", "g_out", "g_logdet"} - ({"trace", "accept"} if call is _bwd else set())
        required = "g_in" if call is _bwd else "z_out"
        for family in (0, 1, 2):
            for name in ptrs:
                if name == "table" and not family:                   # TwoMoons takes a NULL table
                    assert call(L, sfx, family=0, table=None, **{required: None}) == 1
                    assert call(L, sfx, family=0, table=None, b=0) == 0
                    continue
                if name not in optional:
                    assert call(L, sfx, family=family, **{name: None}) == 1, name          # NULL required pointer
                if name != "accept":                                                       # bytes
                    assert call(L, sfx, family=family, **{name: ODD}) == 3, name           # misaligned buffer
            assert call(L, sfx, family=family, b=-1) == 2 and call(L, sfx, family=family, steps=-1) == 2
            assert call(L, sfx, family=family, k=0) == 2 and call(L, sfx, family=family, k=-3) == 2
            assert call(L, sfx, family=family, b=0) == 0 and call(L, sfx, family=family, b=0, steps=0) == 0
            assert call(L, sfx, family=family, b=0, **{p: None for p in ptrs}) == 0        # empty batch: no pointer is read
            assert call(L, sfx, family=family, b=0, k=256, steps=255) == 0                 # 65536 points: the limit
            assert call(L, sfx, family=family, b=0, k=256, steps=256) == 5
            assert call(L, sfx, family=family, k=1 << 17, steps=0) == 5
            assert call(L, sfx, family=family, steps=(1 << 31) - 1) == 5
            # the order: shape before the limit, the limit before a NULL pointer, NULL before alignment
            assert call(L, sfx, family=family, b=-1, steps=65536, beta=None) == 2
            assert call(L, sfx, family=family, steps=65536, k=1, beta=None) == 5
            assert call(L, sfx, family=family, beta=None, prior_loc=ODD) == 1
        for family in (1, 2):
            assert call(L, sfx, family=family, n=0) == 2 and call(L, sfx, family=family, n=-5) == 2
        for family in (3, -1, 1 << 20):
            assert call(L, sfx, family=family) == 5 and call(L, sfx, family=family, b=0) == 5
    assert _bwd(L, sfx, groups=0) == 2 and _bwd(L, sfx, groups=2) == 2 and _bwd(L, sfx, b=1 << 20, groups=1025) == 2
    assert _bwd(L, sfx, b=257, groups=2, workspace=None) == 1 and _bwd(L, sfx, b=257, groups=2, beta=None) == 1


def test_wrappers_refuse_cpu_tensors_shapes_and_dtypes():
    """Before any launch: the wrappers check devices, shapes and dtypes on the host."""
    for device in ("cpu", "meta"):                                   # neither is the GPU: refused whatever else holds
        f = lambda *shape: torch.ones(*shape, device=device)
        with pytest.raises(nf.VcnfError):
            _lib.hmc_annealed_stack(f(4, 2), f(2, 4, 2), f(2, 4), f(2, 2), f(2, 2), f(2, 2), f(2), f(2), f(2), 3, _lib.TARGET_TWO_MOONS)
    with pytest.raises(nf.VcnfError):
        _lib.hmc_annealed_stack_bwd(torch.ones(2, 4, 2), torch.ones(2, 4, dtype=torch.uint8), torch.ones(2, 4, 2), torch.ones(2, 2),
                                    torch.ones(2, 2), torch.ones(2, 2), torch.ones(2), torch.ones(2), torch.ones(2), 3,
                                    _lib.TARGET_TWO_MOONS)
    # the operand checks themselves, on tensors that pass for device tensors of one device
    z = torch.ones(4, 2)
    assert _lib._annealing("t", (torch.ones(2), torch.ones(2), torch.ones(2)), z, 2)[0].shape == (2,)
    for bad in ((torch.ones(3), torch.ones(2), torch.ones(2)), (torch.ones(2, 1), torch.ones(2), torch.ones(2)),
                (torch.ones(2), torch.ones(3), torch.ones(2)), (torch.ones(2), torch.ones(2), torch.ones(1, 2)),
                (torch.ones(2, dtype=torch.float64), torch.ones(2), torch.ones(2)),
                (torch.ones(2), torch.ones(2), torch.ones(2, dtype=torch.float64)), (0.5, torch.ones(2), torch.ones(2)),
                (torch.ones(2), torch.ones(2, device="meta"), torch.ones(2))):
        with pytest.raises(nf.VcnfError):
            _lib._annealing("t", bad, z, 2)


# ---------------------------------------------------------------- the modules
def test_linear_interpolation_and_hais_structure():
    D = nf.distributions
    assert D.linear_interpolation.LinearInterpolation is D.LinearInterpolation and nf.sampling.hais.HAIS is nf.sampling.HAIS
    assert not issubclass(D.LinearInterpolation, torch.nn.Module) and not issubclass(nf.sampling.HAIS, torch.nn.Module)
    prior, target = D.DiagGaussian(2), D.TwoMoons()
    bridge = D.LinearInterpolation(target, prior, 0.25)
    assert bridge.dist1 is target and bridge.dist2 is prior and bridge.alpha == 0.25
    ls, lm = sref.hmc_parameters(0.1)[0]
    layer = nf.flows.HamiltonianMonteCarlo(bridge, 3, ls.float(), lm.float())
    assert [k for k, _ in layer.named_parameters()] == ["log_step_size", "log_mass"]       # not the prior's
    assert list(layer.state_dict()) == ["log_step_size", "log_mass"]

    m = 6
    betas = href.betas_of(m, torch.float32)
    step_size, log_mass = torch.tensor([0.1, 0.12]), torch.tensor([0.1, -0.2])
    sampler = nf.sampling.HAIS(betas, prior, target, 5, step_size, log_mass)
    assert sampler.prior is prior and sampler.target is target and sampler.fuse is True
    assert nf.sampling.HAIS(betas, prior, target, 5, step_size, log_mass, fuse=False).fuse is False
    with pytest.raises(TypeError):
        nf.sampling.HAIS(betas, prior, target, 5, step_size, log_mass, False)               # keyword only
    assert len(sampler.layers) == m - 1
    for j, layer in enumerate(sampler.layers):
        assert type(layer) is nf.flows.HamiltonianMonteCarlo and layer.steps == 5
        assert type(layer.target) is D.LinearInterpolation and layer.target.dist1 is target and layer.target.dist2 is prior
        assert float(layer.target.alpha) == float(betas[m - 1 - j])                         # betas[n - 1] ... betas[1]
        assert torch.equal(layer.log_step_size.detach(), torch.log(step_size)) and torch.equal(layer.log_mass.detach(), log_mass)
        assert len(list(layer.parameters())) == 2
    assert float(sampler.layers[0].target.alpha) == float(betas[m - 1]) and float(sampler.layers[-1].target.alpha) == float(betas[1])


@pytest.mark.parametrize("case", href.CASES, ids=case_id)
def test_cpu_hais_is_the_restatement(case):
    """CPU tensors, a plain-torch prior and a Target subclass that is none of the kernel targets: the composition as the
    reference writes it, the restatement's chain bit for bit in fp64 under one seed, whatever ``fuse`` says."""
    family, n, steps, step = case
    target, prior = sref.plain_target(family, n), href.PlainPrior()
    z = href.inputs(family, n, 65)[1]
    bridge = nf.distributions.LinearInterpolation(target, prior, 0.375)
    assert torch.equal(bridge.log_prob(z), href.bridge_log_prob(family, n, z, 0.375))
    betas = href.betas_of(href.MS[0])
    step_size = torch.tensor([step, 1.2 * step], dtype=torch.float64)
    log_mass = torch.tensor([0.1, -0.2], dtype=torch.float64)
    torch.manual_seed(17)
    want, want_w = href.hais(family, n, betas, 65, steps, step_size, log_mass)
    for fuse in (True, False):
        sampler = nf.sampling.HAIS(betas, prior, target, steps, step_size, log_mass, fuse=fuse)
        torch.manual_seed(17)
        with torch.no_grad():
            got, got_w = sampler.sample(65)
        assert got.dtype == torch.float64 and torch.equal(got, want) and torch.equal(got_w, want_w)
    # and the loop with its draws as arguments is the same chain
    torch.manual_seed(17)
    eps = torch.randn(65, 2, dtype=torch.float64)
    k = href.MS[0] - 1
    noise, unif = torch.empty(k, 65, 2, dtype=torch.float64), torch.empty(k, 65, dtype=torch.float64)
    for j in range(k):
        noise[j] = torch.randn(65, 2, dtype=torch.float64)
        unif[j] = torch.rand(65, dtype=torch.float64)
    x = prior.loc + torch.exp(prior.log_scale) * eps
    params = [(torch.log(step_size), log_mass)] * k
    again, again_w, accept, _ = href.hais_weights(family, n, x, prior.log_prob(x), noise, unif, params, steps, href.layer_betas(href.MS[0]))
    assert torch.equal(again, want) and float((again_w - want_w).abs().max()) <= 1e-12 * float(want_w.abs().max())
    assert 0 < int(accept.sum()) <= accept.numel()


# ---------------------------------------------------------------- the closed-form backward
@pytest.mark.parametrize("case", href.CASES, ids=case_id)
def test_closed_form_backward_is_autograd(case):
    """The VJP of include/vcnf_hip.h with score_k in place of the score against fp64 autograd of the restatement, the
    M = 4 chain at B = 1000: 1e-10 of each tensor's largest entry."""
    family, n, steps, step = case
    m = href.MS[0]
    r = href.reference(*case, 1000, m)
    accept, betas = r[torch.float64][2], list(r["betas"])
    g = torch.Generator().manual_seed(target_ref.seed_of("hais-cotangent", case))
    gz, gl = torch.randn(1000, 2, generator=g, dtype=torch.float64), torch.randn(1000, generator=g, dtype=torch.float64)
    z = r["z"].clone().requires_grad_(True)
    params = [(ls.clone().requires_grad_(True), lm.clone().requires_grad_(True)) for ls, lm in r["params"]]
    out, ld, mask, _ = href.chain(family, n, z, r["noise"], r["unif"], params, steps, betas)
    assert torch.equal(mask, accept) and 0.05 < float(accept.double().mean()) < 1.0
    leaves = [z] + [t for pair in params for t in pair]
    want = torch.autograd.grad((out * gz).sum() + (ld * gl).sum(), leaves)
    got_z, got_params = href.closed_form_backward(family, n, r["z"], r["noise"], r["params"], steps, betas, accept, gz, gl)
    got = [got_z] + [t for pair in got_params for t in pair]
    for name, a, b in zip(["g_z"] + ["g_%s[%d]" % (p, k) for k in range(m - 1) for p in ("log_step_size", "log_mass")], got, want):
        err, top = float((a - b).abs().max()), float(b.abs().max())
        print("%s %s: max error %.3e of %.3e" % (case_id(case), name, err, top))
        assert top > 0 and err <= 1e-10 * top, "%s: %.3e > 1e-10 * %.3e" % (name, err, top)


# ---------------------------------------------------------------- near ties
def test_near_ties():
    """Every case's pooled share of decisions in the band is under the cap, each batch satisfies few_near with its K
    decisions per row, no probability is non-finite, the restatement's fp32 and fp64 chains decide alike outside the
    band, and fp32 can tell every decision there (hais_ref.fp32_resolves; hais_ref.SALTS says which seeds these two
    properties of the restatement chose)."""
    worst = ratios = 0.0
    for case in href.CASES:
        for b, m in href.runs_of(case):
            r = href.reference(*case, b, m)
            k = m - 1
            assert torch.isfinite(r[torch.float64][3]).all() and torch.isfinite(r[torch.float32][3]).all()
            differ = (r[torch.float32][2] != r[torch.float64][2]).any(0) & ~r["near"]
            print("%s B=%d K=%d: %d rows near, accepted per layer %s %%" % (
                case_id(case), b, k, int(r["near"].sum()), [round(100 * float(a), 1) for a in r[torch.float64][2].double().mean(1)]))
            assert not differ.any(), "%s B=%d K=%d: %d rows outside the band decided differently" % (case_id(case), b, k, int(differ.sum()))
            assert sref.few_near(r["near"], k), "%s B=%d K=%d: %d rows in the band" % (case_id(case), b, k, int(r["near"].sum()))
            resolved, ratio = href.fp32_resolves(r)
            ratios = max(ratios, ratio)
            assert resolved, "%s B=%d K=%d: the fp32 restatement is %.3f of a margin from the fp64 one" % (case_id(case), b, k, ratio)
        share = href.band_share(case)
        worst = max(worst, share)
        print("%s: %.2f %% of the decisions in the band" % (case_id(case), 100 * share))
        assert share <= sref.BAND_CAP, "%s: %.2f %% of the decisions in the band" % (case_id(case), 100 * share)
    print("largest share in the band: %.2f %%; largest |prob32 - prob64| / |prob64 - unif| outside it: %.3f" % (100 * worst, ratios))
