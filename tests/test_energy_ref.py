"""The energy densities without a GPU, the Python side: the classes of vcnf_amd.distributions.prior carry the
reference's names, attributes and defaults and are plain objects; on CPU tensors they evaluate the torch composition,
which is the restatement (energy_ref.py) in fp32 and fp64, on the reference's other input shapes too, and is
differentiable; the constant table's cache follows reassigned attributes; the planner admits exactly the five types.
The restatement itself is pinned in fp64: the closed-form scores of include/vcnf_hip.h against autograd, logaddexp
against the reference's log(exp a + exp b) where that is finite, the closed-form backward of the HMC run against
autograd, and the share of the tests' decisions that fall near a tie."""
import pytest
import torch

import energy_ref as eref
import vcnf_amd as nf
from helpers import assert_close, parity
from vcnf_amd import _lib, fused_stochastic

D = nf.distributions
IDS = ["fp32", "fp64"]


def test_classes_attributes_and_defaults():
    assert D.prior.TwoModes is D.TwoModes and D.prior.PriorDistribution is D.PriorDistribution
    for cls in (D.TwoModes, D.Sinusoidal, D.Sinusoidal_gap, D.Sinusoidal_split, D.Smiley):
        assert issubclass(cls, D.PriorDistribution) and not issubclass(cls, torch.nn.Module)
    with pytest.raises(NotImplementedError):
        D.PriorDistribution()
    with pytest.raises(NotImplementedError):
        D.PriorDistribution.log_prob(object.__new__(D.PriorDistribution), torch.zeros(3, 2))
    t = D.TwoModes(2.0, 0.2)
    assert (t.loc, t.scale) == (2.0, 0.2) and vars(t).keys() >= {"loc", "scale"}
    s = D.Sinusoidal(0.4, 4.0)
    assert (s.scale, s.period) == (0.4, 4.0)
    g = D.Sinusoidal_gap(0.4, 4.0)
    assert (g.scale, g.period, g.w2_amp, g.w2_mu, g.w2_scale) == (0.4, 4.0, 3.0, 1.0, 0.6)
    p = D.Sinusoidal_split(0.4, 4.0)
    assert (p.scale, p.period, p.w3_amp, p.w3_mu, p.w3_scale) == (0.4, 4.0, 3.0, 1.0, 0.3)
    assert D.Smiley(0.2).scale == 0.2
    assert (eref.GAP, eref.SPLIT) == ((3.0, 1.0, 0.6), (3.0, 1.0, 0.3))
    for obj in (t, s, g, p, D.Smiley(0.2)):
        with pytest.raises(nf.VcnfError):                # the score is the kernel's alone
            obj.score(torch.zeros(3, 2))


def test_fixed_rows():
    z = eref.inputs(eref.CASES[0], 1000)[0]
    assert z[:10].tolist() == [list(r) for r in eref.FIXED_ROWS] and len(eref.FIXED_ROWS) == 10
    assert eref.inputs(eref.CASES[0], 1)[0].tolist() == [[0.0, 0.0]]
    gap = ("gap", (0.4, 4.0))
    a, b, _ = eref._branches(gap, torch.tensor([[1.0, -2.0], [1.0, -0.5]], dtype=torch.float64))
    assert abs(float(b[0])) < 1e-28 and float(a[0]) < -20.0          # on the second ridge: d + w = 0 up to sin's rounding
    assert float(a[1]) == float(b[1])                                 # both branches equal
    # Smiley's kink: the score of its |.| term is exactly 0, so score1 is the ring term's alone, -(r - 2) / c^2 z1 / r
    kink = z[7:8]
    r = float(torch.sqrt((kink ** 2).sum()))
    for s in (eref.score(("smiley", (0.2,)), kink), eref.closed_form_score(("smiley", (0.2,)), kink)):
        assert abs(float(s[0, 1]) - (-(r - 2) / 0.16 * (-0.8 / r))) <= 1e-14


@pytest.mark.parametrize("dtype", eref.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", eref.CASES, ids=eref.case_id)
def test_cpu_path_is_the_restatement(case, dtype):
    prior = eref.prior_of(case)
    z, g = eref.inputs(case, 1000)
    want64, _, grad64 = eref.gradients(case, z, g, torch.float64)
    want32, _, grad32 = eref.gradients(case, z, g, torch.float32)
    x = z.to(dtype).clone().requires_grad_(True)
    got = prior.log_prob(x)
    grad, = torch.autograd.grad((got * g.to(dtype)).sum(), x)
    assert got.dtype == dtype and tuple(got.shape) == (1000,) and torch.isfinite(got).all() and torch.isfinite(grad).all()
    if dtype == torch.float64:
        # the same formulas: log1p(e) for log(1 + e) and (z^4).sum for norm(p=4)^4 are the only other roundings
        assert_close(got, want64, rtol=1e-12, atol=1e-12, what="log_prob")
        assert float((grad - grad64).abs().max()) <= 1e-12 * float(grad64.abs().max())
    else:
        parity(got, want32, want64, what="log_prob")
        parity(grad, grad32, grad64, what="gradient")
    half = prior.log_prob(z[:16].to(torch.bfloat16))
    assert half.dtype == torch.bfloat16 and tuple(half.shape) == (16,)


@pytest.mark.parametrize("case", [c for c in eref.CASES if c[0] in ("sinusoidal", "gap", "split")], ids=eref.case_id)
def test_sinusoidal_other_ranks(case):
    """The reference moves the last axis first: any rank evaluates, with the last axis the coordinates."""
    prior = eref.prior_of(case)
    z = eref.inputs(case, 1000)[0][:60]
    flat = prior.log_prob(z)
    assert torch.equal(prior.log_prob(z.reshape(3, 20, 2)), flat.reshape(3, 20))
    assert torch.equal(prior.log_prob(z.reshape(3, 4, 5, 2)), flat.reshape(3, 4, 5))
    assert torch.equal(eref.log_prob(case, z.reshape(3, 20, 2)), eref.log_prob(case, z).reshape(3, 20))
    one = prior.log_prob(z[11])                          # a single point [2]
    assert one.dim() == 0 and float(one) == float(flat[11])


@pytest.mark.parametrize("case", eref.CASES, ids=eref.case_id)
def test_closed_form_scores_are_autograds(case):
    z = eref.inputs(case, 1000)[0]
    want = eref.score(case, z)
    got = eref.closed_form_score(case, z)
    assert torch.isfinite(want).all() and torch.isfinite(got).all()
    err, largest = float((got - want).abs().max()), float(want.abs().max())
    print("%s: max |closed form - autograd| %.3e of %.3e" % (eref.case_id(case), err, largest))
    assert err <= 1e-12 * largest
    if case[0] in ("two_modes", "smiley"):
        assert got[0].tolist()[0] == 0.0 == want[0].tolist()[0]          # r == 0
    if case[0] == "two_modes":
        assert float(want[6, 0]) == 0.0 and float(got[6, 0]) == 0.0       # z0 == -0.: the bracket is 0 there


@pytest.mark.parametrize("case", [("gap", (0.4, 4.0)), ("split", (0.4, 4.0))], ids=eref.case_id)
def test_logaddexp_is_the_reference_where_that_is_finite(case):
    z = eref.inputs(case, 1000)[0]
    scale, period = case[1]
    d = z[:, 1] - torch.sin(2 * torch.pi / period * z[:, 0])
    rows = d.abs() <= 10 * scale
    assert 100 < int(rows.sum()) < 1000
    got, naive = eref.log_prob(case, z[rows]), eref.naive_log_prob(case, z[rows])
    assert torch.isfinite(naive).all()
    assert float((got - naive).abs().max()) <= 1e-12 * max(1.0, float(naive.abs().max()))
    # what the departure is for: in fp32 the reference's form is -inf on rows the max-subtracted one keeps finite
    z32 = z.float()
    assert torch.isinf(eref.naive_log_prob(case, z32)).any() and torch.isfinite(eref.log_prob(case, z32)).all()
    assert torch.isfinite(eref.prior_of(case).log_prob(z32)).all()


def test_constant_table_follows_reassigned_attributes(monkeypatch):
    """_operands on host tensors (the device check set aside): the cast is served again while the parameters stand and
    is made anew after an attribute is reassigned."""
    monkeypatch.setattr(_lib, "require_device", lambda *a, **kw: None)
    z32, z64 = torch.zeros(3, 2), torch.zeros(3, 2, dtype=torch.float64)
    gap = D.Sinusoidal_gap(0.4, 4.0)
    table, scale = gap._operands(z32)
    assert table.dtype == torch.float32 and scale == 0.4
    assert table.tolist() == torch.tensor([4.0, 3.0, 1.0, 0.6]).tolist()
    assert gap._operands(z32)[0] is table and gap._operands(z64)[0].dtype == torch.float64
    gap.scale = 0.5
    assert gap._operands(z32)[1] == 0.5
    gap.period, gap.w2_mu = 3.0, 0.5
    table2, _ = gap._operands(z32)
    assert table2 is not table and table2.tolist() == torch.tensor([3.0, 3.0, 0.5, 0.6]).tolist()
    assert gap._operands(z64)[0].tolist() == [3.0, 3.0, 0.5, 0.6] and len(gap._cast) == 2      # one slot per dtype and device
    modes = D.TwoModes(-1.5, 0.3)
    assert modes._operands(z64)[0].tolist() == [-1.5] and modes._operands(z64)[1] == 0.3
    modes.loc = 2
    assert modes._operands(z64)[0].tolist() == [2.0]
    assert D.Smiley(0.2)._operands(z32) == (None, 0.2)
    for bad in (D.Smiley(0.0), D.Sinusoidal(0.0, 4.0), D.Sinusoidal_split(0.4, 0.0), D.TwoModes(2.0, 0)):
        with pytest.raises(ValueError):
            bad._operands(z32)
    # the targets' shared end still serves theirs
    ring = D.RingMixture(2)
    table, scale = ring._operands(z32)
    assert table.tolist() == [1.0, 2.0] and scale == 0.125 and ring._operands(z32)[0] is table
    assert D.TwoMoons()._operands(z32) == (None, 0.0)


def test_planner_admits_exactly_the_five_types():
    for case in eref.CASES:
        assert fused_stochastic.kernel_target(eref.prior_of(case))

    class Mine(D.TwoModes):
        pass

    class Wavy(D.Sinusoidal_gap):
        def log_prob(self, z):
            return super().log_prob(z) * 2
    assert not fused_stochastic.kernel_target(Mine(2.0, 0.2)) and not fused_stochastic.kernel_target(Wavy(0.4, 4.0))
    assert not fused_stochastic.kernel_target(eref.PlainEnergy(eref.CASES[0]))
    assert fused_stochastic.kernel_target(D.TwoMoons())
    # on host tensors the layers take their torch composition, against a prior too
    layer = nf.flows.HamiltonianMonteCarlo(D.Smiley(0.2), 2, torch.log(torch.tensor([0.05, 0.05])), torch.zeros(2))
    z = eref.rows(("smiley", (0.2,)), 65).float()
    assert not fused_stochastic.covers(layer, z)
    torch.manual_seed(3)
    out, ld = layer(z)
    assert tuple(out.shape) == (65, 2) and torch.isfinite(out).all() and torch.isfinite(ld).all()


@pytest.mark.parametrize("case", eref.FAMILIES, ids=eref.case_id)
def test_closed_form_backward_is_autograd(case):
    """energy_ref.hmc_backward, the yardstick of the kernel's VJP, against autograd of the run with the same decisions
    imposed, plain and annealed, in fp64."""
    steps, step = eref.HMC_STEPS[1]
    for annealed in (False, True):
        r = eref.hmc_reference(case, steps, step, 65, eref.RUN, annealed)
        k = len(r["params"])
        accept = r[torch.float64][2]
        g = torch.Generator().manual_seed(5)
        gz, gl = torch.randn(65, 2, generator=g, dtype=torch.float64), torch.randn(65, generator=g, dtype=torch.float64)
        z = r["z"].clone().requires_grad_(True)
        params = [(ls.clone().requires_grad_(True), lm.clone().requires_grad_(True)) for ls, lm in r["params"]]
        dens = eref.densities(case, k, r["betas"])
        out, ld, _, _ = eref.hmc_run(dens, z, r["noise"], None, params, steps, accept=accept)
        want = torch.autograd.grad((out * gz).sum() + (ld * gl).sum(), [z] + [t for pair in params for t in pair])
        g_z, grads = eref.hmc_backward(dens, r["z"], r["noise"], r["params"], steps, accept, gz, gl)
        got = [g_z] + [t for pair in grads for t in pair]
        for a, w in zip(got, want):
            assert float((a - w).abs().max()) <= 1e-10 * max(1.0, float(w.abs().max()))


@pytest.mark.parametrize("case", eref.CASES, ids=eref.case_id)
def test_hmc_near_ties(case):
    """The conditions of the GPU tests' decision comparisons, on the restatement alone: a case's pooled share of
    decisions in the band under the cap, every batch comparing something, no fp32-vs-fp64 decision differing outside
    the band, and rejections exercised at the larger step."""
    for annealed in (False, True):
        for steps, step in eref.HMC_STEPS:
            share, rejected, differ = eref.hmc_band_share(case, steps, step, annealed)
            print("%s steps %d step %g annealed %s: %.2f %% in the band, %.1f %% rejected, %d fp32 decisions differ outside it"
                  % (eref.case_id(case), steps, step, annealed, 100 * share, 100 * rejected, differ))
            assert share <= eref.BAND_CAP and differ == 0
            if not annealed:
                assert (0.05 < rejected < 0.5) if steps == 4 else rejected < 0.02
            for b, k in eref.hmc_runs(annealed):
                near = eref.hmc_reference(case, steps, step, b, k, annealed)["near"]
                assert eref.few_near(near, k), (b, k, int(near.sum()))


@pytest.mark.parametrize("case", eref.CASES, ids=eref.case_id)
def test_mh_near_ties(case):
    for steps in eref.MH_STEPS:
        for scale in eref.MH_SCALES:
            share = eref.mh_band_share(case, steps, scale)
            differ = 0
            for b in eref.MH_BATCHES:
                r = eref.mh_reference(case, steps, scale, b)
                assert eref.few_near(r["near"]), (b, int(r["near"].sum()))
                differ += int(((r[torch.float32][1] != r[torch.float64][1]).any(0) & ~r["near"]).sum())
            print("%s steps %d scale %s: %.2f %% of rows in the band, %d fp32 rows differ outside it" % (eref.case_id(case), steps, scale, 100 * share, differ))
            assert share <= eref.BAND_CAP and differ == 0
