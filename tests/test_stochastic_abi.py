"""The stochastic layers without a GPU: the vcnf_hmc_stack_* / vcnf_hmc_stack_bwd_* / vcnf_mh_walk_* symbols are
exported and bound and return the documented status codes before anything is launched; the modules carry the
reference's parameter, buffer and state_dict names and are their own inverses; their torch path on CPU tensors with a
plain Target subclass is the restatement (stochastic_ref.py) bit for bit under one seed, which pins the order of the
draws; the closed-form backward of include/vcnf_hip.h, written in torch, is fp64 autograd of the restatement; and the
near-tie bands the GPU tests leave out are as thin as they assume, with the restatement's own fp32 and fp64 runs deciding
alike outside them."""
import ctypes

import pytest
import torch

import stochastic_ref as sref
import target_ref
import vcnf_amd as nf
from vcnf_amd import _lib

FAKE = ctypes.c_void_p(0x1000)         # never dereferenced: validation fails first / batch == 0
ODD = ctypes.c_void_p(0x1002)          # not aligned to a float or a double
NAMES = ("vcnf_hmc_stack", "vcnf_hmc_stack_bwd", "vcnf_mh_walk")
case_id = lambda c: "-".join(str(x) for x in c) if isinstance(c, tuple) else str(c)


def test_symbols_exported_and_bound():
    handle = ctypes.CDLL(_lib.lib_path())
    for base in NAMES:
        for sfx, real in (("_f32", ctypes.c_float), ("_f64", ctypes.c_double)):
            name = base + sfx
            assert hasattr(handle, name), "libvcnf_hip.so does not export " + name
            assert name in _lib.PROTOTYPES and getattr(nf.lib(), name).argtypes == _lib.PROTOTYPES[name][0]
            assert _lib.PROTOTYPES[name][0][-2] is real                  # the target's scale, before the stream
    assert len(_lib.PROTOTYPES["vcnf_hmc_stack_f32"][0]) == 18 and len(_lib.PROTOTYPES["vcnf_hmc_stack_bwd_f32"][0]) == 22
    assert len(_lib.PROTOTYPES["vcnf_mh_walk_f32"][0]) == 13
    assert callable(_lib.hmc_stack) and callable(_lib.hmc_stack_bwd) and callable(_lib.mh_walk)
    assert issubclass(nf.autograd.HmcStackFn, torch.autograd.Function)


HMC_PTRS = ("z", "noise", "unif", "step", "mass", "sqrt_mass", "table", "z_out", "log_det", "trace", "accept")
BWD_PTRS = ("trace", "accept", "noise", "step", "mass", "sqrt_mass", "table", "g_out", "g_logdet", "g_in", "g_step", "g_mass",
            "g_sqrt_mass", "workspace")
MH_PTRS = ("z", "eps", "w", "prop_scale", "table", "z_out", "accept")


def _hmc(L, sfx, b=4, k=2, steps=3, n=3, family=1, **ptrs):
    return getattr(L, "vcnf_hmc_stack" + sfx)(*[ptrs.get(p, FAKE) for p in HMC_PTRS], b, k, steps, n, family, 0.5, None)


def _bwd(L, sfx, b=4, k=2, steps=3, groups=1, n=3, family=1, **ptrs):
    return getattr(L, "vcnf_hmc_stack_bwd" + sfx)(*[ptrs.get(p, FAKE) for p in BWD_PTRS], b, k, steps, groups, n, family, 0.5, None)


def _mh(L, sfx, b=4, steps=3, n=3, family=1, **ptrs):
    return getattr(L, "vcnf_mh_walk" + sfx)(*[ptrs.get(p, FAKE) for p in MH_PTRS], b, steps, n, family, 0.5, None)


@pytest.mark.parametrize("sfx", ["_f32", "_f64"])
def test_validation_status_codes(sfx):
    L = nf.lib()
    optional = {"trace", "accept", "g_out", "g_logdet"}
    unaligned_ok = {"accept"}                                            # bytes
    for call, ptrs, layered in ((_hmc, HMC_PTRS, True), (_bwd, BWD_PTRS, True), (_mh, MH_PTRS, False)):
        one = dict(k=1) if layered else {}
        optional_here = optional - ({"trace", "accept"} if call is _bwd else set())
        for family in (0, 1, 2):
            for name in ptrs:
                if name == "table" and not family:
                    _two_moons_ignores_table(call, L, sfx)
                    continue
                if name not in optional_here:
                    assert call(L, sfx, family=family, **{name: None}) == 1, name          # NULL required pointer
                if name not in unaligned_ok:
                    assert call(L, sfx, family=family, **{name: ODD}) == 3, name           # misaligned buffer
            assert call(L, sfx, family=family, b=-1) == 2
            assert call(L, sfx, family=family, steps=-1) == 2
            assert call(L, sfx, family=family, b=0) == 0                 # empty batch: no launch
            assert call(L, sfx, family=family, b=0, steps=0) == 0        # steps == 0 is legal
            assert call(L, sfx, family=family, b=0, **{p: None for p in ptrs}) == 0
            if layered:
                assert call(L, sfx, family=family, k=0) == 2 and call(L, sfx, family=family, k=-3) == 2
                assert call(L, sfx, family=family, b=0, k=256, steps=255) == 0             # 65536 points: the limit
                assert call(L, sfx, family=family, b=0, k=256, steps=256) == 5
                assert call(L, sfx, family=family, k=1 << 17, steps=0) == 5
            assert call(L, sfx, family=family, b=0, steps=65535, **one) == 0
            assert call(L, sfx, family=family, steps=65536, **one) == 5
            assert call(L, sfx, family=family, steps=(1 << 31) - 1) == 5
        for family in (1, 2):
            assert call(L, sfx, family=family, n=0) == 2 and call(L, sfx, family=family, n=-5) == 2
        assert call(L, sfx, family=0, n=-1, table=None, z_out=None, g_in=None) == 1       # TwoMoons ignores n_comp too
        for family in (3, -1, 1 << 20):
            assert call(L, sfx, family=family) == 5 and call(L, sfx, family=family, b=0) == 5
    # the VJP's workgroup count: one block of the workspace each, none without a tile of 256 samples
    assert _bwd(L, sfx, groups=0) == 2 and _bwd(L, sfx, groups=-1) == 2 and _bwd(L, sfx, groups=2) == 2
    assert _bwd(L, sfx, b=257, groups=3) == 2 and _bwd(L, sfx, b=1 << 20, groups=1025) == 2
    assert _bwd(L, sfx, b=257, groups=2, workspace=None) == 1 and _bwd(L, sfx, b=1 << 20, groups=1024, g_in=None) == 1


def _two_moons_ignores_table(call, L, sfx):
    """TwoMoons takes a NULL table: the call gets past that check and stops at the next thing wrong with it."""
    required = "g_in" if call is _bwd else "z_out"
    assert call(L, sfx, family=0, table=None, **{required: None}) == 1
    assert call(L, sfx, family=0, table=None, **{required: ODD}) == 3
    assert call(L, sfx, family=0, table=None, b=0) == 0


# ---------------------------------------------------------------- the modules
def _hmc_module(target, steps=3, numel=2):
    ls, lm = sref.hmc_parameters(0.1, 1, numel)[0]
    return nf.flows.HamiltonianMonteCarlo(target, steps, ls.float(), lm.float())


def test_module_names_and_state_dicts():
    D, F = nf.distributions, nf.flows
    assert F.stochastic.HamiltonianMonteCarlo is F.HamiltonianMonteCarlo and F.stochastic.MetropolisHastings is F.MetropolisHastings
    assert D.mh_proposal.MHProposal is D.MHProposal and D.mh_proposal.DiagGaussianProposal is D.DiagGaussianProposal
    for numel in (1, 2):
        hmc = _hmc_module(D.TwoMoons(), numel=numel)
        assert isinstance(hmc, F.Flow) and hmc.steps == 3 and isinstance(hmc.target, D.TwoMoons)
        assert [k for k, _ in hmc.named_parameters()] == ["log_step_size", "log_mass"]
        assert hmc.log_step_size.numel() == hmc.log_mass.numel() == numel
        assert list(hmc.state_dict()) == ["log_step_size", "log_mass", "target.prop_scale", "target.prop_shift"]
    hmc = _hmc_module(D.CircularGaussianMixture())
    assert list(hmc.state_dict()) == ["log_step_size", "log_mass", "target.prop_scale", "target.prop_shift", "target.scale"]
    other = _hmc_module(D.CircularGaussianMixture())
    other.load_state_dict(hmc.state_dict())

    base = D.MHProposal()
    for call in (lambda: base.sample(torch.zeros(2, 2)), lambda: base.log_prob(torch.zeros(2, 2), torch.zeros(2, 2)),
                 lambda: base(torch.zeros(2, 2))):
        with pytest.raises(NotImplementedError):
            call()
    prop = D.DiagGaussianProposal((2,), [0.3, 0.24])
    assert isinstance(prop, D.MHProposal) and prop.shape == (2,) and not list(prop.parameters())
    assert list(prop.state_dict()) == ["scale"] and tuple(prop.scale.shape) == (1, 2) and prop.scale.dtype == torch.float32
    assert tuple(D.DiagGaussianProposal((2,), 0.5).scale.shape) == (1,)
    torch.manual_seed(3)
    z = torch.randn(5, 2, dtype=torch.float64)
    torch.manual_seed(4)
    z_, diff = prop(z)
    torch.manual_seed(4)
    assert torch.equal(z_, prop.sample(z)) and z_.dtype == torch.float64 and torch.equal(diff, torch.zeros(5, dtype=torch.float64))
    torch.manual_seed(4)
    assert torch.equal(z_, torch.randn(5, 2, dtype=torch.float64) * prop.scale + z)
    prop64 = D.DiagGaussianProposal((2,), [0.3, 0.24]).double()          # log(scale) in the buffer's own precision
    want = torch.distributions.Normal(z, prop64.scale.expand(5, 2)).log_prob(z_).sum(1)
    assert float((prop64.log_prob(z_, z) - want).abs().max()) < 1e-12

    mh = F.MetropolisHastings(D.RingMixture(), prop, 4)
    assert isinstance(mh, F.Flow) and mh.steps == 4 and mh.proposal is prop and not list(mh.parameters())
    assert list(mh.state_dict()) == ["dist.prop_scale", "dist.prop_shift", "proposal.scale"]

    model = nf.NormalizingFlow(D.DiagGaussian(2), [_hmc_module(D.TwoMoons())], D.TwoMoons())
    assert model.fuse_stochastic_stacks is True
    assert [k for k, _ in model.named_parameters()][-2:] == ["flows.0.log_step_size", "flows.0.log_mass"]


def test_kernel_targets_refuse_cpu_tensors():
    """With a kernel target there is no CPU path: the layer reaches target.log_prob, which refuses the tensor."""
    D = nf.distributions
    z = torch.zeros(3, 2)
    with pytest.raises(nf.VcnfError):
        _hmc_module(D.TwoMoons())(z)
    with pytest.raises(nf.VcnfError):
        nf.flows.MetropolisHastings(D.TwoMoons(), D.DiagGaussianProposal((2,), [0.3, 0.24]), 2)(z)
    for bad in (torch.zeros(3, 2), torch.zeros(3, 3, device="meta")):
        with pytest.raises(nf.VcnfError):
            _lib.mh_walk(bad, torch.zeros(1, 3, 2), torch.zeros(1, 3), torch.zeros(2), _lib.TARGET_TWO_MOONS)


# ---------------------------------------------------------------- the torch path is the restatement
@pytest.mark.parametrize("dtype", sref.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("case", sref.HMC_CASES, ids=case_id)
def test_hmc_torch_path_is_the_restatement(case, dtype):
    family, n, steps, step = case
    z = sref.inputs(family, n, 65).to(dtype)
    for numel in (1, 2):
        ls, lm = (t.to(dtype) for t in sref.hmc_parameters(step, 1, numel)[0])
        layer = nf.flows.HamiltonianMonteCarlo(sref.plain_target(family, n), steps, ls.clone(), lm.clone())
        for call in (layer.forward, layer.inverse):                      # inverse is forward
            torch.manual_seed(11)
            with torch.no_grad():
                out, ld = call(z)
            torch.manual_seed(11)
            noise = torch.randn_like(z)
            unif = torch.rand(len(z), dtype=dtype)
            want, want_ld, accept, _ = sref.hmc_layer(family, n, z, noise, unif, ls, lm, steps)
            assert out.dtype == dtype and torch.equal(out, want) and torch.equal(ld, want_ld)
            assert torch.equal(out[~accept], z[~accept]) and int(accept.sum()) > 0
    # under autograd: gradients reach z and both parameters, through the detached score
    x = z.clone().requires_grad_(True)
    torch.manual_seed(11)
    out, ld = layer(x)
    (out.sum() + ld.sum()).backward()
    assert torch.isfinite(x.grad).all() and bool((layer.log_step_size.grad != 0).any()) and bool((layer.log_mass.grad != 0).any())


@pytest.mark.parametrize("dtype", sref.DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("scale", sref.MH_SCALES, ids=case_id)
@pytest.mark.parametrize("target", sref.TARGETS, ids=case_id)
def test_mh_torch_path_is_the_restatement(target, scale, dtype):
    family, n = target
    z = sref.inputs(family, n, 65).to(dtype)
    for steps in (0,) + sref.MH_STEPS:
        prop = nf.distributions.DiagGaussianProposal((2,), list(scale)).to(dtype)
        layer = nf.flows.MetropolisHastings(sref.plain_target(family, n), prop, steps)
        for call in (layer.forward, layer.inverse):
            torch.manual_seed(13)
            out, ld = call(z)
            torch.manual_seed(13)
            eps, w = torch.empty(steps, 65, 2, dtype=dtype), torch.empty(steps, 65, dtype=dtype)
            for i in range(steps):                                       # per step: the proposal's randn, then rand
                eps[i] = torch.randn(65, 2, dtype=dtype)
                w[i] = torch.rand(65, dtype=dtype)
            want, want_ld, accept, _ = sref.mh_walk(family, n, z, eps, w, prop.scale[0])
            assert out.dtype == dtype and torch.equal(out, want) and torch.equal(ld, want_ld) and not ld.any()
        x = z.clone().requires_grad_(True)
        gz = torch.randn(65, 2, dtype=dtype)
        out, _ = layer(x)
        grad, = torch.autograd.grad((out * gz).sum(), x)
        assert torch.equal(grad, gz)                                     # the identity under differentiation


# ---------------------------------------------------------------- the closed-form backward
@pytest.mark.parametrize("case", sref.HMC_CASES, ids=case_id)
def test_closed_form_backward_is_autograd(case):
    """The VJP of include/vcnf_hip.h in torch against fp64 autograd of the restatement, a run of three layers at
    B = 1000: 1e-10 of each tensor's largest entry."""
    family, n, steps, step = case
    r = sref.hmc_reference(family, n, steps, step, 1000, sref.RUN)
    accept = r[torch.float64][2]
    g = torch.Generator().manual_seed(target_ref.seed_of("cotangent", case))
    gz, gl = torch.randn(1000, 2, generator=g, dtype=torch.float64), torch.randn(1000, generator=g, dtype=torch.float64)
    z = r["z"].clone().requires_grad_(True)
    params = [(ls.clone().requires_grad_(True), lm.clone().requires_grad_(True)) for ls, lm in r["params"]]
    out, ld, mask, _ = sref.hmc_run(family, n, z, r["noise"], r["unif"], params, steps)
    assert torch.equal(mask, accept) and 0.05 < float(accept.double().mean()) < 1.0
    leaves = [z] + [t for pair in params for t in pair]
    want = torch.autograd.grad((out * gz).sum() + (ld * gl).sum(), leaves)
    got_z, got_params = sref.hmc_closed_form_backward(family, n, r["z"], r["noise"], r["params"], steps, accept, gz, gl)
    got = [got_z] + [t for pair in got_params for t in pair]
    for name, a, b in zip(["g_z"] + ["g_%s[%d]" % (p, k) for k in range(sref.RUN) for p in ("log_step_size", "log_mass")], got, want):
        err, top = float((a - b).abs().max()), float(b.abs().max())
        print("%s %s: max error %.3e of %.3e" % (case_id(case), name, err, top))
        assert top > 0 and err <= 1e-10 * top, "%s: %.3e > 1e-10 * %.3e" % (name, err, top)


# ---------------------------------------------------------------- near ties
def _hmc_gpu_cases():
    return [(c, b, 1) for c in sref.HMC_CASES for b in sref.BATCHES] + [(c, 1000, sref.RUN) for c in sref.HMC_CASES]


def test_hmc_near_ties():
    """Measured here: at most 0.8 % of a case's decisions lie in the band |min(prob, 2) - unif| < 1e-2 (2 % allowed), and
    the restatement's fp32 and fp64 runs decide alike on every row outside it, in every batch and run of the GPU tests.
    The share is taken over the case's batches and layers together (stochastic_ref.hmc_band_share says why); each single
    batch leaves out at most 2 rows where B <= 65 and never all of its rows (stochastic_ref.few_near)."""
    worst = 0.0
    for case in sref.HMC_CASES:
        for _, b, k in [c for c in _hmc_gpu_cases() if c[0] == case]:
            r = sref.hmc_reference(*case, b, k)
            differ = (r[torch.float32][2] != r[torch.float64][2]).any(0) & ~r["near"]
            print("%s B=%d K=%d: %d rows near, accepted %.1f %%" % (case_id(case), b, k, int(r["near"].sum()),
                                                                   100 * float(r[torch.float64][2].double().mean())))
            assert not differ.any(), "%s B=%d K=%d: %d rows outside the band decided differently" % (case_id(case), b, k, int(differ.sum()))
            assert sref.few_near(r["near"], k), "%s B=%d K=%d: %d rows in the band" % (case_id(case), b, k, int(r["near"].sum()))
        share = sref.hmc_band_share(*case)
        worst = max(worst, share)
        assert share <= sref.BAND_CAP, "%s: %.2f %% of the decisions in the band" % (case_id(case), 100 * share)
    print("largest share in the band: %.2f %%" % (100 * worst))
    assert worst <= 0.008


def test_mh_near_ties():
    """Measured here: at most 0.9 % of a case's rows have a step within 1e-3 of a tie (2 % allowed); none outside decided
    differently by the restatement's fp32 and fp64 runs."""
    worst = 0.0
    for family, n in sref.TARGETS:
        for steps in sref.MH_STEPS:
            for scale in sref.MH_SCALES:
                for b in sref.MH_BATCHES:
                    r = sref.mh_reference(family, n, steps, scale, b)
                    differ = (r[torch.float32][2] != r[torch.float64][2]).any(0) & ~r["near"]
                    assert not differ.any(), "%s-%d steps %d B=%d: %d rows outside the band decided differently" % (
                        family, n, steps, b, int(differ.sum()))
                    assert sref.few_near(r["near"]), "%s-%d steps %d B=%d: %d rows in the band" % (family, n, steps, b, int(r["near"].sum()))
                share = sref.mh_band_share(family, n, steps, scale)
                worst = max(worst, share)
                assert share <= sref.BAND_CAP, "%s-%d steps %d: %.2f %% in the band" % (family, n, steps, 100 * share)
    print("largest share in the band: %.2f %%" % (100 * worst))
    assert worst <= 0.009
